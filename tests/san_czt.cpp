// The host side of Transforms.czt (csrc/czt_plan.hpp) in a stand-alone program for ASan / UBSan: the argument checks over a sweep with
// the rejected ones, the tier choice and the convolution length at their edges, the phase reduction against exact integer arithmetic,
// the table builder against the Bluestein identity it serves (a naive double sum), the spread against a walk over the tables, and the
// row and lane arithmetic of the fused kernel walked lane by lane over heap buffers of exactly the size the C entry point is promised —
// a load or a store outside them is the sanitizer's to report.  Built and run by tests/test_czt_host.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "czt_plan.hpp"

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

static const CztContour kUnit{1.0, 1.0, 13, 1.0, 0.0};

static void test_checks_and_tier() {
  bool u = false;
  struct Case { int32_t cplx; int64_t length, batch, stride, m; CztContour c; const char* frag; bool unsupported; };
  const double inf = INFINITY, nan = NAN;
  const Case bad[] = {
      {2, 8, 1, 8, 8, kUnit, "is_complex", false},                              {0, 0, 1, 8, 8, kUnit, "length must be >= 1", false},
      {0, 8, 1, 8, 0, kUnit, "m must be >= 1", false},                          {0, 8, -1, 8, 8, kUnit, "batch must be >= 0", false},
      {0, 8, 2, 7, 8, kUnit, "batch_stride must be >= length", false},          {0, 8, 1, 8, 8, {1.0, 1.0, 0, 1.0, 0.0}, "w_den must be >= 1", false},
      {0, 8, 1, 8, 8, {0.0, 1.0, 1, 1.0, 0.0}, "w_abs", false},                 {0, 8, 1, 8, 8, {inf, 1.0, 1, 1.0, 0.0}, "w_abs", false},
      {0, 8, 1, 8, 8, {nan, 1.0, 1, 1.0, 0.0}, "w_abs", false},                 {0, 8, 1, 8, 8, {1.0, 1.0, 1, -2.0, 0.0}, "a_abs", false},
      {0, 8, 1, 8, 8, {1.0, nan, 1, 1.0, 0.0}, "w_step must be finite", false}, {0, 8, 1, 8, 8, {1.0, 1.0, 1, 1.0, inf}, "a_turns must be finite", false},
      {0, 8, 1, 8, ((int64_t)1 << 30) - 6, kUnit, "2^30", true},                {0, ((int64_t)1 << 30) + 1, 1, ((int64_t)1 << 30) + 1, 1, kUnit, "2^30", true},
      {0, 8, 1, 8, 8, {1.0, 1.0, (int64_t)1 << 62, 1.0, 0.0}, "w_den must be at most", true},
      {1, 8, 16, (int64_t)1 << 59, 8, kUnit, "too large", true},                {0, 8, (int64_t)1 << 40, 8, 8, kUnit, "too large", true},
  };
  for (const Case& c : bad) {
    const char* what = czt_check(c.cplx, c.length, c.batch, c.stride, c.m, c.c, &u);
    CHECK(what && std::strstr(what, c.frag) && u == c.unsupported, "check(%d, %lld, %lld, %lld, %lld) said %s", c.cplx, (long long)c.length,
          (long long)c.batch, (long long)c.stride, (long long)c.m, what ? what : "nothing");
  }
  CHECK(!czt_check(0, 8, 0, 8, 8, kUnit, &u) && !u, "batch = 0 is valid");
  CHECK(!czt_check(1, 1, 1, 1, 1, kUnit, &u), "one sample, one point");
  CHECK(!czt_check(0, 48000, 8, 48000, 4096, kUnit, &u), "8 x 1 s at 48 kHz");
  // the edges n + m - 1 = 1024, 1025, 2048, 2049
  struct Edge { int64_t n, m, L; int tier; };
  const Edge edges[] = {{1, 1, 1024, kCzWave},    {512, 513, 1024, kCzWave},      {513, 513, 2048, kCzWave},  {1024, 1, 1024, kCzWave},
                        {1024, 1025, 2048, kCzWave}, {1025, 1025, 4096, kCzGeneric}, {2048, 1, 2048, kCzWave},   {2049, 1, 4096, kCzGeneric},
                        {1, 2049, 4096, kCzGeneric}, {5000, 37, 8192, kCzGeneric},   {40000, 64, 65536, kCzGeneric}};
  for (const Edge& e : edges) {
    CHECK(czt_tier(e.n, e.m, false) == e.tier && czt_conv_length(e.n, e.m, false) == e.L, "tier / L of (%lld, %lld)", (long long)e.n, (long long)e.m);
    CHECK(czt_tier(e.n, e.m, true) == kCzGeneric, "the switch at (%lld, %lld)", (long long)e.n, (long long)e.m);
    const int64_t L = czt_conv_length(e.n, e.m, true);
    CHECK(czt_is_pow2(L) && L >= czt_need(e.n, e.m) && (L == 1 || L / 2 < czt_need(e.n, e.m)), "generic L of (%lld, %lld)", (long long)e.n, (long long)e.m);
  }
  CHECK(czt_waves(1024) == 4 && czt_waves(2048) == 2, "waves per workgroup");
  CHECK(czt_lds_bytes(1024) == 45568 && czt_lds_bytes(2048) == 53504, "LDS per workgroup");
  int a = 0;
  CHECK(czt_overlap(&a, 4, &a, 4) && !czt_overlap(&a, 0, &a, 4) && !czt_overlap(&a, 4, &a + 1, 4) && czt_overlap(&a, 8, &a + 1, 4), "overlap");
}

// frac(mult * value / den) against exact integer arithmetic, where 128 bits hold it: value = num / 2^t with small num
static void test_phase_reduction() {
  for (int t : {0, 1, 7, 20, 52}) {
    for (int64_t num : {(int64_t)1, (int64_t)3, (int64_t)-5, (int64_t)1000003, (int64_t)-999983}) {
      const double value = std::ldexp((double)num, -t);
      for (uint64_t den : {(uint64_t)1, (uint64_t)2, (uint64_t)26, (uint64_t)4096, (uint64_t)10000019, (uint64_t)1 << 40}) {
        const czt_u128 f = czt_turn_fraction(value, den);
        for (uint64_t j : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)1023, (uint64_t)65537, ((uint64_t)1 << 20) - 1, ((uint64_t)1 << 31) - 1}) {
          const czt_u128 j2 = (czt_u128)j * j;
          // exactly: frac(j^2 num / (den 2^t)), the remainder taken in 128-bit integers (j^2 |num| < 2^62 2^20, den 2^t < 2^92)
          const czt_u128 D = (czt_u128)den << t;
          const czt_u128 mag = j2 * (czt_u128)(uint64_t)(num < 0 ? -num : num) % D;
          const czt_u128 rem = (num < 0 && mag != 0) ? D - mag : mag;
          const double want = (double)rem / (double)D;                             // in [0, 1)
          double got = czt_angle(j2 * f) / 6.283185307179586476925286766559;       // in [-1/2, 1/2)
          double d = got - want;
          d -= std::nearbyint(d);
          CHECK(std::fabs(d) <= 1e-15, "frac(%llu^2 * %g / %llu) = %.17g, exactly %.17g", (unsigned long long)j, value, (unsigned long long)den, got, want);
        }
      }
    }
  }
  CHECK(czt_turn_fraction(0.0, 7) == 0 && czt_turn_fraction(3.0, 1) == 0 && czt_turn_fraction(-8.0, 2) == 0, "whole turns");
  CHECK(czt_turn_fraction(0.5, 1) == (czt_u128)1 << 127 && czt_turn_fraction(1.0, 4) == (czt_u128)1 << 126, "a half and a quarter");
  CHECK(czt_turn_fraction(-0.25, 1) == (czt_u128)3 << 126, "minus a quarter");
  // 2^300 = 1 mod 3, so a third of a turn: floor(2^128 / 3) = (2^128 - 1) / 3
  CHECK(czt_turn_fraction(std::ldexp(1.0, -200), 1) == 0 && czt_turn_fraction(std::ldexp(1.0, 300), 3) == ~(czt_u128)0 / 3, "the far ends of the exponent");
  CHECK(czt_turn_fraction(5e-324, 1) == 0, "a denormal");
}

// W . IDFT(DFT(x A) F) L = the definition, by naive sums in double; and the spread against the tables' own magnitudes
static void test_tables(int64_t n, int64_t m, int64_t L, const CztContour& c) {
  std::vector<double> A((size_t)2 * n), F((size_t)2 * L), W((size_t)2 * m);
  double spread = 0.0;
  const char* what = czt_tables(n, m, L, c, A.data(), F.data(), W.data(), &spread);
  CHECK(!what, "tables(%lld, %lld, %lld): %s", (long long)n, (long long)m, (long long)L, what ? what : "");
  if (what) return;
  typedef std::complex<double> cd;
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<cd> x((size_t)n), z((size_t)L, cd(0.0)), Z((size_t)L), y((size_t)L);
  for (int64_t j = 0; j < n; ++j) { x[j] = cd(0.25 * ((j * 37) % 11) - 1.0, 0.5 * ((j * 17) % 7) - 1.5); z[j] = x[j] * cd(A[2 * j], A[2 * j + 1]); }
  for (int64_t k = 0; k < L; ++k) {
    cd acc = 0.0;
    for (int64_t j = 0; j < n; ++j) acc += z[j] * std::polar(1.0, -two_pi * (double)(j * k % L) / (double)L);
    Z[k] = acc * cd(F[2 * k], F[2 * k + 1]);
  }
  const cd w = std::polar(c.w_abs, -two_pi * c.w_step / (double)c.w_den), a = std::polar(c.a_abs, two_pi * c.a_turns);
  double top = 0.0, worst = 0.0;
  std::vector<cd> want((size_t)m);
  for (int64_t k = 0; k < m; ++k) {
    cd acc = 0.0;
    for (int64_t j = 0; j < n; ++j) acc += x[j] * std::pow(a, -(double)j) * std::pow(w, (double)(j * k));
    want[k] = acc;
    if (std::abs(acc) > top) top = std::abs(acc);
  }
  for (int64_t k = 0; k < m; ++k) {
    cd acc = 0.0;
    for (int64_t q = 0; q < L; ++q) acc += Z[q] * std::polar(1.0, two_pi * (double)(q * k % L) / (double)L);
    const cd got = acc * cd(W[2 * k], W[2 * k + 1]);
    if (std::abs(got - want[k]) > worst) worst = std::abs(got - want[k]);
  }
  CHECK(worst <= 1e-10 * top, "tables(%lld, %lld, %lld): the identity misses the definition by %g of %g", (long long)n, (long long)m, (long long)L, worst, top);
  double lo = 1.0, hi = 1.0, seen = 1.0;
  for (int64_t j = 0; j < n; ++j) { const double v = std::hypot(A[2 * j], A[2 * j + 1]); if (v < lo) lo = v; if (v > hi) hi = v; }
  seen = hi / lo; lo = hi = 1.0;
  for (int64_t k = 0; k < m; ++k) { const double v = std::hypot(W[2 * k], W[2 * k + 1]); if (v < lo) lo = v; if (v > hi) hi = v; }
  if (hi / lo > seen) seen = hi / lo;
  const double J = (double)((n > m ? n : m) - 1), lv = std::exp(std::fabs(0.5 * J * J * std::log(c.w_abs)));
  if (lv > seen) seen = lv;
  CHECK(std::fabs(spread - seen) <= 1e-9 * seen && spread <= kCztSpreadGate, "spread %g, the tables show %g", spread, seen);
}

// the fused kernel's walk: workgroups of W waves over chunks of rows, every lane loading its pairs and storing its outputs, over buffers
// of exactly ((batch - 1) stride + n) samples and batch * m results; the tables are the padded ones of L entries
static void walk(int L, int64_t n, int64_t m, int64_t batch, int64_t stride, bool cplx, int rows_per_wave) {
  bool u = false;
  CHECK(!czt_check(cplx, n, batch, stride, m, kUnit, &u) && czt_tier(n, m, false) == kCzWave && czt_conv_length(n, m, false) == L, "walk arguments");
  const int W = czt_waves(L), NQ = L / 128, P = L / 64, per = cplx ? 2 : 1;
  const int64_t chunk = (int64_t)W * rows_per_wave, blocks = czt_blocks(batch, chunk);
  std::vector<float> x((size_t)((batch - 1) * stride + n) * per);
  for (size_t i = 0; i < x.size(); ++i) x[i] = (float)(i % 251) + 1.0f;
  std::vector<float> out((size_t)batch * m * 2, 0.0f), table((size_t)L * 2, 1.0f);
  std::vector<int> reads((size_t)batch * n, 0), writes((size_t)batch * m, 0), bins((size_t)L, 0);
  for (int64_t b = 0; b < blocks; ++b)
    for (int wave = 0; wave < W; ++wave) {
      int64_t r_end = (b + 1) * chunk;
      if (r_end > batch) r_end = batch;
      for (int64_t r = b * chunk + wave; r < r_end; r += W)
        for (int lane = 0; lane < 64; ++lane) {
          for (int q = 0; q < NQ; ++q) {
            const int i0 = czt_slot_sample(lane, q), st = czt_pair_state(i0, (int)n);
            const float* row = x.data() + (size_t)r * stride * per;
            const float t0 = table[2 * (size_t)i0], t1 = table[2 * (size_t)i0 + 3];   // the pair's two entries: one 16-byte load
            float v0 = 0.0f, v1 = 0.0f;
            if (st >= 1) { v0 = row[(size_t)i0 * per] * t0; ++reads[(size_t)r * n + i0]; }
            if (st == 2) { v1 = row[(size_t)(i0 + 1) * per + (per - 1)] * t1; ++reads[(size_t)r * n + i0 + 1]; }
            const int so = czt_pair_state(i0, (int)m);
            float* o = out.data() + ((size_t)r * m + i0) * 2;
            if (so >= 1) { o[0] = v0; o[1] = v0; ++writes[(size_t)r * m + i0]; }
            if (so == 2) { o[2] = v1; o[3] = v1; ++writes[(size_t)r * m + i0 + 1]; }
          }
          if (r == 0)
            for (int s = 0; s < P; ++s) ++bins[(size_t)czt_bin(lane, s)];
        }
    }
  for (size_t i = 0; i < reads.size(); ++i) CHECK(reads[i] == 1, "L %d n %lld: sample %zu read %d times", L, (long long)n, i, reads[i]);
  for (size_t i = 0; i < writes.size(); ++i) CHECK(writes[i] == 1, "L %d m %lld: output %zu written %d times", L, (long long)m, i, writes[i]);
  for (size_t i = 0; i < bins.size(); ++i) CHECK(bins[i] == 1, "L %d: bin %zu multiplied %d times", L, i, bins[i]);
  for (int64_t r = 0; r < batch; ++r)
    for (int64_t i = 0; i < m; ++i) {
      const float want = i < n ? x[((size_t)r * stride + i) * per + ((i & 1) ? per - 1 : 0)] : 0.0f;
      CHECK(out[((size_t)r * m + i) * 2] == want, "L %d row %lld index %lld: the walk carried %g, the row holds %g", L, (long long)r, (long long)i,
            out[((size_t)r * m + i) * 2], want);
    }
  // the alignment rule: wide only where two adjacent elements start on twice the element size
  for (uint64_t addr = 0; addr < 64; addr += 4) {
    CHECK(czt_wide(addr, 4) == (addr % 8 == 0), "f32 rows at %llu", (unsigned long long)addr);
    if (addr % 8 == 0) CHECK(czt_wide(addr, 8) == (addr % 16 == 0), "c64 rows at %llu", (unsigned long long)addr);
  }
}

int main() {
  test_checks_and_tier();
  test_phase_reduction();
  test_tables(1, 1, 1, kUnit);
  test_tables(3, 7, 16, {1.0, 1.0, 7, 1.0, 0.0});
  test_tables(20, 13, 32, {1.0, 0.4, 13, 1.0, 0.05});
  test_tables(20, 13, 64, {1.0, 0.058887, 1, 1.0, 0.031831});
  test_tables(33, 17, 64, {1.002, 0.0175, 1, 0.995, 0.047746});
  test_tables(17, 33, 64, {0.998, -0.0175, 1, 1.004, -0.3});
  double sp = 0.0;
  std::vector<double> A(128), F(256), W(128);
  CHECK(czt_tables(64, 64, 128, {1.01, 0.1, 1, 1.0, 0.0}, A.data(), F.data(), W.data(), &sp) != nullptr && sp > kCztSpreadGate, "a spiral beyond the gate");
  CHECK(!(czt_spread(1000, 1000, {2.0, 0.1, 1, 1.0, 0.0}) <= kCztSpreadGate), "a spread beyond double");
  for (int64_t batch : {1, 2, 3, 65})
    for (int64_t gap : {0, 5})
      for (bool cplx : {false, true})
        for (int rpw : {1, 4}) {
          for (auto nm : {std::pair<int64_t, int64_t>{1, 1}, {3, 7}, {600, 300}, {512, 513}, {1000, 25}, {1, 1024}, {1024, 1}, {127, 129}})
            walk(1024, nm.first, nm.second, batch, nm.first + gap, cplx, rpw);
          for (auto nm : {std::pair<int64_t, int64_t>{513, 513}, {1024, 1025}, {1500, 549}, {2048, 1}, {1, 2048}, {25, 1501}})
            walk(2048, nm.first, nm.second, batch, nm.first + gap, cplx, rpw);
        }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitized czt host side ok\n");
  return 0;
}
