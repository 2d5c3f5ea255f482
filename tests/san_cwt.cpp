// The host side of Transforms.cwt / Filters.fir_bank (csrc/cwt_plan.hpp) in a stand-alone program, built with ASan / UBSan by
// tests/test_cwt_host.py: the support rule and the wavelets at their edges, the argument checks over accepted and refused banks, the
// class split and the block geometry at N = 513 | 514 and 1025 | 1026, and the fused kernel's block, lane and slot arithmetic walked over
// exactly sized buffers — every load inside the row, every output of every filter written exactly once — with the overlap-save scheme
// carried out in double (cwt_spectrum and a direct circular convolution) against the definition.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cwt_plan.hpp"

using namespace nxsig;

static int g_checks = 0;
#define REQUIRE(cond)                                                      \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// the definition in double: out[n] = full[n + (N - 1) / 2]
static std::vector<double> same_direct(const std::vector<double>& x, const std::vector<double>& h /* interleaved */, int64_t N) {
  const int64_t L = (int64_t)x.size(), c = cwt_center(N);
  std::vector<double> out((size_t)2 * L, 0.0);
  for (int64_t n = 0; n < L; ++n)
    for (int64_t j = 0; j < N; ++j) {
      const int64_t k = n + c - j;
      if (k < 0 || k >= L) continue;
      out[2 * n] += x[k] * h[2 * j]; out[2 * n + 1] += x[k] * h[2 * j + 1];
    }
  return out;
}

// one class of a bank through the kernel's arithmetic: blocks, lanes, slots; the circular convolution done directly with the filter
// placed as cwt_spectrum places it
static void walk_class(const std::vector<double>& x, const std::vector<std::vector<double>>& bank, const std::vector<int64_t>& counts, int K) {
  const int64_t L = (int64_t)x.size();
  const int64_t Nmax = *std::max_element(counts.begin(), counts.end());
  const int64_t step = cwt_step(K, Nmax), lead = cwt_lead(Nmax), bpr = cwt_blocks_per_row(L, step);
  REQUIRE(step >= K / 2 - 1 && step >= 1);
  const int NQ = K / 128;
  for (size_t f = 0; f < bank.size(); ++f) {
    const int64_t N = counts[f], c = cwt_center(N);
    // the filter placed circularly, as cwt_spectrum does
    std::vector<double> g((size_t)2 * K, 0.0);
    for (int64_t j = 0; j < N; ++j) {
      const int64_t at = ((j - c) % K + K) % K;
      g[2 * at] += bank[f][2 * j]; g[2 * at + 1] += bank[f][2 * j + 1];
    }
    std::vector<double> out((size_t)2 * L, 0.0);
    std::vector<int> written((size_t)L, 0);
    for (int64_t b = 0; b < bpr; ++b) {
      const int64_t base = cwt_block_base(b, step, lead);
      std::vector<double> blk((size_t)K, 0.0);
      std::vector<int> loaded((size_t)K, 0);
      for (int lane = 0; lane < 64; ++lane)
        for (int q = 0; q < NQ; ++q)
          for (int par = 0; par < 2; ++par) {
            const int t = cwt_slot_pos(lane, q) + par;
            REQUIRE(t >= 0 && t < K);
            ++loaded[t];
            const int64_t i = base + t;
            if (i >= 0 && i < L) blk[t] = x.at((size_t)i);   // at(): a load outside the row aborts
          }
      for (int t = 0; t < K; ++t) REQUIRE(loaded[t] == 1);
      for (int t = 0; t < K; ++t) {
        if (!cwt_pos_valid(t, base, lead, step, L)) continue;
        double re = 0.0, im = 0.0;
        for (int64_t i = 0; i < K; ++i) {
          if (g[2 * i] == 0.0 && g[2 * i + 1] == 0.0) continue;
          const double s = blk[(size_t)(((t - i) % K + K) % K)];
          re += s * g[2 * i]; im += s * g[2 * i + 1];
        }
        const int64_t n = base + t;
        out.at((size_t)(2 * n)) = re; out.at((size_t)(2 * n + 1)) = im;
        ++written.at((size_t)n);
      }
    }
    for (int64_t n = 0; n < L; ++n) REQUIRE(written[n] == 1);
    const std::vector<double> ref = same_direct(x, bank[f], N);
    double top = 0.0, err = 0.0;
    for (size_t i = 0; i < ref.size(); ++i) { top = std::max(top, std::fabs(ref[i])); err = std::max(err, std::fabs(ref[i] - out[i])); }
    REQUIRE(err <= 1e-12 * (top > 0.0 ? top : 1.0));
  }
  int bins[2048] = {};
  for (int lane = 0; lane < 64; ++lane)
    for (int s = 0; s < K / 64; ++s) ++bins[cwt_bin(lane, s)];
  for (int k = 0; k < K; ++k) REQUIRE(bins[k] == 1);
}

int main() {
  // ---- the support rule
  REQUIRE(cwt_support(0.1, 100) == 1 && cwt_support(1.0, 100) == 10 && cwt_support(2.5, 100) == 25 && cwt_support(4.5, 100) == 45);
  REQUIRE(cwt_support(10.0, 37) == 37 && cwt_support(1e300, 5) == 5 && cwt_support(1e-300, 5) == 1 && cwt_support(0.35, 100) == 4);
  REQUIRE(cwt_support(51.3, 5000) == 513 && cwt_support(51.4, 5000) == 514 && cwt_support(102.5, 5000) == 1025 && cwt_support(102.6, 5000) == 1026);
  // ---- the wavelets: ricker's centre and symmetry, morlet2's conjugate symmetry once reversed, N = 1
  for (int64_t N : {1, 2, 7, 10, 45}) {
    std::vector<double> r((size_t)2 * N), m((size_t)2 * N);
    cwt_wavelet(kCwRicker, 1.7, 5.0, N, r.data());
    cwt_wavelet(kCwMorlet2, 1.7, 5.0, N, m.data());
    for (int64_t j = 0; j < N; ++j) {
      REQUIRE(r[2 * j + 1] == 0.0 && std::fabs(r[2 * j] - r[2 * (N - 1 - j)]) <= 1e-15);
      REQUIRE(std::fabs(m[2 * j] - m[2 * (N - 1 - j)]) <= 1e-15 && std::fabs(m[2 * j + 1] + m[2 * (N - 1 - j) + 1]) <= 1e-15);
    }
    REQUIRE(cwt_all_finite(r.data(), 2 * N) && cwt_all_finite(m.data(), 2 * N));
  }
  // ---- the checks
  bool unsupported = true;
  REQUIRE(cwt_rows_check(8, 1, 8, kCwPower, &unsupported) == nullptr && !unsupported);
  REQUIRE(cwt_rows_check(8, 0, 8, 0, &unsupported) && cwt_rows_check(8, 65536, 8, 0, &unsupported) && cwt_rows_check(0, 1, 8, 0, &unsupported));
  REQUIRE(cwt_rows_check(8, 1, 7, 0, &unsupported) && cwt_rows_check(8, 1, 8, 4, &unsupported) && cwt_rows_check(8, 1, 8, -1, &unsupported));
  {
    int64_t total = 0, longest = 0;
    const int64_t ok[3] = {3, 1, 9}, zero[3] = {3, 0, 9}, big[2] = {1, kCwtMaxExtent};
    REQUIRE(cwt_bank_check(8, 0, ok, 3, &total, &longest, &unsupported) == nullptr && total == 13 && longest == 9);
    REQUIRE(cwt_bank_check(8, 2, ok, 3, &total, &longest, &unsupported) && !unsupported);
    REQUIRE(cwt_bank_check(8, 0, ok, 0, &total, &longest, &unsupported) && cwt_bank_check(8, 0, ok, 4097, &total, &longest, &unsupported));
    REQUIRE(cwt_bank_check(8, 0, zero, 3, &total, &longest, &unsupported) && !unsupported);
    REQUIRE(cwt_bank_check(2, 0, big, 2, &total, &longest, &unsupported) && unsupported);
    REQUIRE(cwt_bank_check(1, 0, big, 2, &total, &longest, &unsupported) == nullptr);
    const double good[2] = {0.5, 3.0}, bad0[2] = {0.5, 0.0}, badn[2] = {NAN, 1.0}, badi[2] = {1.0, INFINITY};
    REQUIRE(cwt_widths_check(kCwMorlet2, good, 2, 5.0) == nullptr && cwt_widths_check(kCwRicker, good, 2, NAN) == nullptr);
    REQUIRE(cwt_widths_check(kCwMorlet2, good, 2, NAN) && cwt_widths_check(2, good, 2, 5.0) && cwt_widths_check(0, good, 0, 5.0));
    REQUIRE(cwt_widths_check(0, bad0, 2, 5.0) && cwt_widths_check(0, badn, 2, 5.0) && cwt_widths_check(0, badi, 2, 5.0));
  }
  // ---- the classes and the block geometry at their edges
  REQUIRE(cwt_class(1, false) == kCwWave1024 && cwt_class(513, false) == kCwWave1024 && cwt_class(514, false) == kCwWave2048);
  REQUIRE(cwt_class(1025, false) == kCwWave2048 && cwt_class(1026, false) == kCwGeneric && cwt_class(1, true) == kCwGeneric);
  REQUIRE(cwt_step(1024, 513) == 512 && cwt_step(1024, 1) == 1024 && cwt_step(2048, 1025) == 1024 && cwt_step(2048, 514) == 1535);
  REQUIRE(cwt_lead(1) == 0 && cwt_lead(2) == 1 && cwt_lead(3) == 1 && cwt_lead(513) == 256 && cwt_lead(514) == 257);
  REQUIRE(cwt_generic_length(5000, 1026) == 8192 && cwt_generic_length(1, 1) == 1 && cwt_generic_length(4096, 2) == 8192);
  REQUIRE(cwt_lds_bytes(1024) == 45568 && cwt_lds_bytes(2048) == 53504);
  {
    const int64_t counts[7] = {10, 513, 514, 1025, 1026, 1, 3000};
    CwtGroups g;
    cwt_split(counts, 7, false, &g);
    REQUIRE(g.members[kCwWave1024] == (std::vector<int32_t>{0, 1, 5}) && g.longest[kCwWave1024] == 513);
    REQUIRE(g.members[kCwWave2048] == (std::vector<int32_t>{2, 3}) && g.longest[kCwWave2048] == 1025);
    REQUIRE(g.members[kCwGeneric] == (std::vector<int32_t>{4, 6}) && g.longest[kCwGeneric] == 3000);
    cwt_split(counts, 7, true, &g);
    REQUIRE(g.members[kCwWave1024].empty() && g.members[kCwWave2048].empty() && g.members[kCwGeneric].size() == 7);
  }
  // ---- the kernel's walk: rows shorter than, equal to and longer than a block, banks at the edges of both classes
  unsigned seed = 12345u;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((double)(seed >> 8) / (double)(1u << 24)) - 0.5; };
  struct Shape { int K; int64_t L; std::vector<int64_t> counts; };
  const Shape shapes[] = {{1024, 1, {1}}, {1024, 2, {1, 2}}, {1024, 37, {1, 10, 25, 37}}, {1024, 1537, {1, 10, 45, 100}}, {1024, 1300, {513, 2, 7}},
                          {2048, 1100, {514, 600}}, {2048, 2500, {1025, 514}}, {1024, 1024, {512}}, {1024, 513, {513}}};
  for (const Shape& s : shapes) {
    std::vector<double> x((size_t)s.L);
    for (double& v : x) v = rnd();
    std::vector<std::vector<double>> bank;
    for (int64_t N : s.counts) {
      std::vector<double> h((size_t)2 * N);
      for (double& v : h) v = rnd();
      bank.push_back(h);
    }
    walk_class(x, bank, s.counts, s.K);
  }
  // ---- cwt_spectrum: the spectrum's bin 0 is the sum of the taps (times the scale), and a placement wraps as the walk assumes
  {
    const int64_t N = 5, K = 16;
    const double h[10] = {1, 0.5, 2, -1, 3, 0, 4, 0.25, 5, -2};
    std::vector<double> work;
    std::vector<float> H((size_t)2 * K);
    cwt_spectrum(h, N, K, cwt_center(N), 1.0 / K, work, H.data());
    REQUIRE(std::fabs(H[0] - 15.0f / 16.0f) <= 1e-7 && std::fabs(H[1] - (-2.25f) / 16.0f) <= 1e-7);
    cwt_spectrum(h, N, K, 0, 1.0, work, H.data());
    REQUIRE(std::fabs(H[0] - 15.0f) <= 1e-6);
  }
  REQUIRE(czt_overlap(&seed, 4, &seed, 4));
  // the edges once more as text, for the Python test to read: N -> class, points, step and lead of a class whose longest filter is N
  for (int64_t N : {1, 513, 514, 1025, 1026}) {
    const int cls = cwt_class(N, false), K = cwt_class_points(cls);
    std::printf("edge N=%lld class=%d K=%d step=%lld lead=%lld name=%s\n", (long long)N, cls, K, (long long)cwt_step(K, N), (long long)cwt_lead(N),
                cwt_class_name(cls));
  }
  std::printf("sanitized cwt host side ok: %d checks\n", g_checks);
  return 0;
}
