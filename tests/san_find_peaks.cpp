// The host side of PeakFinding.find_peaks (nx_signal_amd/csrc/find_peaks_plan.hpp) in a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_find_peaks_host.py: the argument checks, the capacity and block arithmetic, every walk
// with the line summary against the same walk element by element (the kernels call these very functions), and the rounds of the
// distance stage against the sequential rule.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "find_peaks_plan.hpp"

using namespace nxsig;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static void checks() {
  char msg[96];
  double b[10];
  for (int k = 0; k < 5; ++k) b[2 * k] = -INFINITY, b[2 * k + 1] = INFINITY;
  auto run = [&](uint32_t cond, const double* bounds, double dist, int64_t wlen, double rel, uint32_t want, int64_t cap, int64_t most) {
    const char* r = find_peaks_check(cond, bounds, dist, wlen, rel, want, cap, most, msg, sizeof msg);
    return std::string(r ? r : "");
  };
  CHECK(run(0, nullptr, 1.0, -1, 0.5, 0, 4, 4) == "");
  CHECK(run(kFpConditionMask, b, 1.0, 2, 0.0, kFpWantMask, 0, 4) == "");
  CHECK(run(kFpDistance, nullptr, 0.5, -1, 0.5, 0, 4, 4) == "`distance` must be greater or equal to 1");
  CHECK(run(kFpDistance, nullptr, NAN, -1, 0.5, 0, 4, 4) == "`distance` must be greater or equal to 1");
  CHECK(run(0, nullptr, 0.5, -1, 0.5, 0, 4, 4) == "");   // no distance condition: the value is not looked at
  CHECK(run(0, nullptr, 1.0, 1, 0.5, 0, 4, 4) == "`wlen` must be larger than 1, was 1");
  CHECK(run(0, nullptr, 1.0, -5, 0.5, 0, 4, 4) == "`wlen` must be larger than 1, was -5");
  CHECK(run(0, nullptr, 1.0, -1, -0.1, 0, 4, 4) == "`rel_height` must be greater or equal to 0.0");
  CHECK(run(0, nullptr, 1.0, -1, NAN, 0, 4, 4) == "`rel_height` must be greater or equal to 0.0");
  CHECK(run(64, nullptr, 1.0, -1, 0.5, 0, 4, 4) == "unknown bits in conditions");
  CHECK(run(0, nullptr, 1.0, -1, 0.5, 1u << 13, 4, 4) == "unknown bits in want");
  CHECK(run(kFpHeight, nullptr, 1.0, -1, 0.5, 0, 4, 4) == "null pointer argument");
  CHECK(run(0, nullptr, 1.0, -1, 0.5, 0, 5, 4) == "capacity must be in [0, lines * ((n - 1) / 2)]");
  CHECK(run(0, nullptr, 1.0, -1, 0.5, 0, -1, 4) == "capacity must be in [0, lines * ((n - 1) / 2)]");
  b[3] = NAN;
  CHECK(run(kFpHeight, b, 1.0, -1, 0.5, 0, 4, 4) == "a border is not a number");

  CHECK(find_peaks_capacity(7, 1) == 0 && find_peaks_capacity(7, 2) == 0 && find_peaks_capacity(7, 3) == 7 && find_peaks_capacity(7, 4) == 7);
  CHECK(find_peaks_capacity(2, 5) == 4 && find_peaks_capacity(1, 2147483647) == 1073741823);
  CHECK(find_peaks_blocks(1) == 1 && find_peaks_blocks(64) == 1 && find_peaks_blocks(65) == 2 && find_peaks_blocks(2147483647) == 33554432);
  CHECK(find_peaks_d(1.0, 10) == 1 && find_peaks_d(7.5, 10) == 8 && find_peaks_d(10.0, 10) == 10 && find_peaks_d(1e300, 10) == 10 &&
        find_peaks_d(INFINITY, 10) == 10);
  CHECK(find_peaks_f64_rows(kFpWantMask) == 8 && find_peaks_s32_rows(kFpWantMask) == 5 && find_peaks_f64_rows(1u << kFpLeftBases) == 0 &&
        find_peaks_s32_rows((1u << kFpLeftBases) | (1u << kFpWidths)) == 1);
  CHECK(fp_within(1.0, -INFINITY, INFINITY) && fp_within(NAN, -INFINITY, INFINITY) && !fp_within(NAN, 0.0, INFINITY) && fp_within(1.0, 1.0, 1.0) &&
        !fp_within(1.0, 1.5, INFINITY) && !fp_within(2.0, -INFINITY, 1.5));
}

// one line of n samples at stride st inside a buffer of the exact size (ASan sees a step past either end), its summary beside it
template <typename T>
struct Case {
  std::vector<T> buf, smin, smax, tmin, tmax;
  FpLine<T> L;
  Case(const std::vector<T>& v, int64_t st) {
    const int64_t n = (int64_t)v.size(), nb = find_peaks_blocks(n), ns = find_peaks_supers(n);
    buf.assign((size_t)((n - 1) * st + 1), (T)777);
    for (int64_t i = 0; i < n; ++i) buf[(size_t)(i * st)] = v[(size_t)i];
    smin.resize((size_t)nb);
    smax.resize((size_t)nb);
    for (int64_t b = 0; b < nb; ++b) fp_block_summary<T>(buf.data(), st, n, b, &smin[(size_t)b], &smax[(size_t)b]);
    tmin.resize((size_t)ns);
    tmax.resize((size_t)ns);
    for (int64_t k = 0; k < ns; ++k) fp_super_summary<T>(smin.data(), smax.data(), 1, nb, k, &tmin[(size_t)k], &tmax[(size_t)k]);
    L.x = buf.data(); L.st = st; L.n = n; L.smin = smin.data(); L.smax = smax.data(); L.tmin = tmin.data(); L.tmax = tmax.data(); L.sst = 1;
  }
};

template <typename T>
static int64_t compare_walks(const std::vector<T>& v, int64_t st) {
  Case<T> c(v, st);
  const FpLine<T>& L = c.L;
  int64_t peaks = 0;
  for (int64_t i = 1; i + 1 < L.n; ++i) {
    int64_t ra = -1, rb = -1;
    const bool a = fp_peak_at<T, true>(L, i, &ra), b = fp_peak_at<T, false>(L, i, &rb);
    CHECK(a == b && ra == rb);
    if (!b) continue;
    ++peaks;
    const int64_t p = (i + rb) / 2;
    const T pv = L.at(p);
    CHECK((fp_plateau_start<T, true>(L, p, pv)) == i && (fp_plateau_start<T, false>(L, p, pv)) == i);
    CHECK((fp_plateau_end<T, true>(L, p, pv)) == rb + 1 && (fp_plateau_end<T, false>(L, p, pv)) == rb + 1);
    for (int64_t half : {(int64_t)-1, (int64_t)1, (int64_t)31, (int64_t)32, (int64_t)64, (int64_t)100, (int64_t)4096, (int64_t)6000, L.n}) {
      const FpProminence x = fp_prominence<T, true>(L, p, half), y = fp_prominence<T, false>(L, p, half);
      CHECK(same(x.prominence, y.prominence) && x.left_base == y.left_base && x.right_base == y.right_base);
      CHECK(y.left_base >= 0 && y.left_base <= p && y.right_base >= p && y.right_base < L.n);
      for (double rel : {0.0, 0.5, 0.7, 1.0, 1.5}) {
        const FpWidth wa = fp_width<T, true>(L, p, x, rel), wb = fp_width<T, false>(L, p, y, rel);
        CHECK(same(wa.width, wb.width) && same(wa.width_height, wb.width_height) && same(wa.left_ip, wb.left_ip) && same(wa.right_ip, wb.right_ip));
      }
    }
  }
  return peaks;
}

template <typename T>
static void walks() {
  std::mt19937_64 rng(12345);
  std::normal_distribution<double> gauss;
  const int B = kFindPeaksBlock;
  int64_t peaks = 0;
  for (int64_t n : {1, 2, 3, 4, 5, B - 1, B, B + 1, 2 * B, 3 * B + 5, 4 * B, 4 * B + 1, 9 * B - 3})
    for (int kind = 0; kind < 6; ++kind)
      for (int64_t st : {1, 3}) {
        std::vector<T> v((size_t)n);
        for (auto& s : v) s = (T)gauss(rng);
        if (kind == 1) for (auto& s : v) s = (T)std::round((double)s);                 // many plateaus and equal minima
        if (kind == 2) for (size_t k = 0; k < v.size(); k += 37) v[k] = (T)NAN;         // NaN here and there
        if (kind == 3) for (size_t k = 0; k < v.size(); ++k) v[k] = (T)(k % 97 == 5 ? INFINITY : k % 89 == 7 ? -INFINITY : (double)v[k]);
        if (kind == 4) {                                                                 // long flats: zeros with a few steps
          for (auto& s : v) s = 0;
          for (size_t k = 0; k < v.size(); k += 150) v[k] = (T)-1;
          if (n > 3 * B) for (int64_t k = B / 2; k < 3 * B - 7; ++k) v[(size_t)k] = 2;   // a plateau from one block into the third
        }
        if (kind == 5) for (size_t k = 0; k < v.size(); ++k) v[k] = (T)(k % 2 ? 1.0 : 0.0) + (k == v.size() / 2 ? (T)5 : (T)0);   // equal minima everywhere
        peaks += compare_walks<T>(v, st);
      }
  // the tallest peak of a 4 B line: bases in the first and the last block, every block between them crossed through the summary
  std::vector<T> v((size_t)(4 * B), (T)1);
  v[3] = 0; v[(size_t)(4 * B - 2)] = (T)0.5; v[(size_t)(2 * B)] = 9;
  for (size_t k = 5; k < v.size() - 3; k += 3) if (k != (size_t)(2 * B)) v[k] = (T)1.5;
  Case<T> c(v, 1);
  const FpProminence pr = fp_prominence<T, true>(c.L, 2 * B, -1);
  CHECK(pr.left_base == 3 && pr.right_base == 4 * B - 2 && same(pr.prominence, 8.5));
  peaks += compare_walks<T>(v, 1);
  // lines longer than a super-block: noise on a slow slope (long walks), flats of several super-blocks, NaN and Inf in the way
  const int64_t S = kFindPeaksSuper;
  for (int64_t n : {S - 1, S, S + 1, 2 * S + 70, 3 * S + 5})
    for (int kind = 0; kind < 4; ++kind) {
      std::vector<T> w((size_t)n);
      for (size_t k = 0; k < w.size(); ++k) w[k] = (T)(std::round(gauss(rng) * 4) / 4 + (kind == 1 ? 0.0 : 1e-3 * (double)k));
      if (kind == 1) {
        for (size_t k = 0; k < w.size(); ++k) w[k] = (T)(k % 1000 == 3 ? -1.0 : 0.0);
        if (n > 2 * S) for (int64_t k = 100; k < 2 * S + 20; ++k) w[(size_t)k] = 2;
      }
      if (kind == 2) w[(size_t)(n / 3)] = (T)NAN, w[(size_t)(n / 2)] = (T)INFINITY;
      if (kind == 3) w[(size_t)(n / 2)] = 50, w[7] = -3, w[(size_t)(n - 9)] = -3;
      peaks += compare_walks<T>(w, kind == 3 ? 2 : 1);
    }
  CHECK(peaks > 5000);
}

static void distance() {
  std::mt19937_64 rng(99);
  int64_t most_rounds = 0;
  for (int trial = 0; trial < 400; ++trial) {
    const int64_t m = 1 + (int64_t)(rng() % 60), d = 1 + (int64_t)(rng() % 12);
    std::vector<double> h((size_t)m);
    std::vector<int64_t> pos((size_t)m);
    int64_t at = 1;
    for (int64_t k = 0; k < m; ++k) {
      at += 2 + (int64_t)(rng() % 4);
      pos[(size_t)k] = at;
      h[(size_t)k] = trial % 3 == 0 ? (double)(rng() % 3) : trial % 3 == 1 ? (double)(rng() % 1000) : 1.0;   // many ties, few ties, all equal
    }
    std::vector<uint8_t> a((size_t)m), b((size_t)m);
    find_peaks_distance_sequential(h.data(), pos.data(), m, d, a.data());
    const int64_t rounds = find_peaks_distance_rounds(h.data(), pos.data(), m, d, b.data());
    CHECK(a == b);
    most_rounds = rounds > most_rounds ? rounds : most_rounds;
  }
  // [0 2 0 2 0 2 0 2 0], d = 3: the larger index is visited first, 7 then 3 survive
  {
    const double h[4] = {2, 2, 2, 2};
    const int64_t pos[4] = {1, 3, 5, 7};
    uint8_t a[4], b[4];
    find_peaks_distance_sequential(h, pos, 4, 3, a);
    find_peaks_distance_rounds(h, pos, 4, 3, b);
    CHECK(!a[0] && a[1] && !a[2] && a[3] && !std::memcmp(a, b, 4));
  }
  // a descending chain at spacing 2 with d = 3: one decision per round and its neighbour, about chain / 2 rounds
  for (int up = 0; up < 2; ++up) {
    const int64_t m = 200;
    std::vector<double> h((size_t)m);
    std::vector<int64_t> pos((size_t)m);
    for (int64_t k = 0; k < m; ++k) pos[(size_t)k] = 1 + 2 * k, h[(size_t)k] = up ? (double)k : (double)(m - k);
    std::vector<uint8_t> a((size_t)m), b((size_t)m);
    find_peaks_distance_sequential(h.data(), pos.data(), m, 3, a.data());
    const int64_t rounds = find_peaks_distance_rounds(h.data(), pos.data(), m, 3, b.data());
    CHECK(a == b && rounds >= m / 2 && rounds <= m / 2 + 1);
    for (int64_t k = 0; k < m; ++k) CHECK(a[(size_t)k] == (up ? (m - 1 - k) % 2 == 0 : k % 2 == 0));
  }
  CHECK(most_rounds >= 2);
}

int main() {
  checks();
  walks<float>();
  walks<double>();
  distance();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("sanitized find_peaks host side ok\n");
  return 0;
}
