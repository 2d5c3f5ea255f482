// The host side of Convolution.correlate_rows / convolve_rows (csrc/xcorr_plan.hpp) in a stand-alone program for ASan / UBSan: the
// argument checks over a sweep with the rejected ones, the tier and the transform length at their edges, the index maps full -> circular
// against a circular correlation / convolution summed directly, SciPy's first lag, the mirror-bin map of the packed split, the row scale
// over every kind of float, the slab arithmetic, and the lane and slot arithmetic of the fused kernel walked lane by lane over heap
// buffers of exactly the size the C entry point is promised — a load or a store outside them is the sanitizer's to report.  Built and
// run by tests/test_xcorr_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xcorr_plan.hpp"

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

static void test_checks_and_tier() {
  bool u = false;
  struct Case { int64_t n1, sa, n2, sb, batch; int32_t cplx, op, mode, w; double floor; int32_t sink; const char* frag; bool unsupported; };
  const int64_t big = (int64_t)1 << 30;
  const Case bad[] = {
      {8, 8, 4, 4, 1, 2, 1, 0, 0, 0.0, 0, "is_complex", false},       {8, 8, 4, 4, 1, 0, 2, 0, 0, 0.0, 0, "op must be", false},
      {8, 8, 4, 4, 1, 0, 1, 3, 0, 0.0, 0, "expected mode", false},    {8, 8, 4, 4, 1, 0, 1, 0, 2, 0.0, 0, "weighting must be", false},
      {8, 8, 4, 4, 1, 0, 1, 0, 0, 0.0, 2, "sink must be", false},     {8, 8, 4, 4, 1, 0, 0, 0, 1, 0.0, 0, "phat weighting belongs", false},
      {8, 8, 4, 4, 1, 0, 0, 0, 0, 0.0, 1, "peak sink belongs", false}, {8, 8, 4, 4, 1, 0, 1, 0, 1, 1.0, 0, "phat_floor", false},
      {8, 8, 4, 4, 1, 0, 1, 0, 1, -0.5, 0, "phat_floor", false},      {8, 8, 4, 4, 1, 0, 1, 0, 1, NAN, 0, "phat_floor", false},
      {0, 8, 4, 4, 1, 0, 1, 0, 0, 0.0, 0, "lengths must be", false},  {8, 8, 0, 4, 1, 0, 1, 0, 0, 0.0, 0, "lengths must be", false},
      {8, 8, 4, 4, -1, 0, 1, 0, 0, 0.0, 0, "batch must be", false},   {8, 7, 4, 4, 2, 0, 1, 0, 0, 0.0, 0, "a_stride must be", false},
      {8, 8, 4, 3, 2, 0, 1, 0, 0, 0.0, 0, "b_stride must be", false}, {8, 8, 4, -1, 2, 0, 1, 0, 0, 0.0, 0, "b_stride must be", false},
      {8, 8, big - 6, 0, 1, 0, 1, 0, 0, 0.0, 0, "2^30", true},        {big + 1, big + 1, 1, 1, 1, 0, 1, 0, 0, 0.0, 0, "2^30", true},
      {8, (int64_t)1 << 59, 4, 4, 16, 1, 1, 0, 0, 0.0, 0, "too large", true}, {8, 8, 4, 4, (int64_t)1 << 40, 0, 1, 0, 0, 0.0, 0, "too large", true},
  };
  for (const Case& c : bad) {
    const char* what = xcorr_check(c.n1, c.sa, c.n2, c.sb, c.batch, c.cplx, c.op, c.mode, c.w, c.floor, c.sink, &u);
    CHECK(what && std::strstr(what, c.frag) && u == c.unsupported, "check(%lld, %lld, ...) said %s, wanted %s", (long long)c.n1, (long long)c.n2,
          what ? what : "nothing", c.frag);
  }
  CHECK(!xcorr_check(8, 8, 4, 4, 0, 0, 1, 0, 0, 0.0, 0, &u) && !u, "batch = 0 is valid");
  CHECK(!xcorr_check(8, 8, 4, 0, 3, 1, 1, 2, 1, 0.5, 1, &u), "a shared template, PHAT and the peak sink");
  CHECK(!xcorr_check(48000, 48000, 48000, 48000, 64, 0, 0, 1, 0, 0.0, 0, &u), "64 x 1 s at 48 kHz");
  // need = 1024, 1025, 2048, 2049
  struct Edge { int64_t n1, n2, P; int real_tier, cplx_tier; };
  const Edge edges[] = {{1, 1, 1024, kXcWave, kXcWave},           {512, 513, 1024, kXcWave, kXcWave},       {1024, 1, 1024, kXcWave, kXcWave},
                        {513, 513, 2048, kXcWave, kXcGeneric},    {1024, 1025, 2048, kXcWave, kXcGeneric},  {2048, 1, 2048, kXcWave, kXcGeneric},
                        {1025, 1025, 4096, kXcGeneric, kXcGeneric}, {2049, 1, 4096, kXcGeneric, kXcGeneric}, {5000, 4000, 16384, kXcGeneric, kXcGeneric},
                        {48000, 48000, 131072, kXcGeneric, kXcGeneric}};
  for (const Edge& e : edges) {
    CHECK(xcorr_fft_length(e.n1, e.n2) == e.P, "P of (%lld, %lld)", (long long)e.n1, (long long)e.n2);
    CHECK(xcorr_tier(e.n1, e.n2, false, false) == e.real_tier && xcorr_tier(e.n1, e.n2, true, false) == e.cplx_tier, "tier of (%lld, %lld)",
          (long long)e.n1, (long long)e.n2);
    CHECK(xcorr_tier(e.n1, e.n2, false, true) == kXcGeneric && xcorr_tier(e.n1, e.n2, true, true) == kXcGeneric, "the switch");
  }
  CHECK(xcorr_fft_length(400, 201) == 1024 && xcorr_tier(400, 201, false, true) == kXcGeneric, "need 600 under the switch: generic at P = 1024");
}

// the circular result at P, summed directly, against the definition's full result through the maps
static void test_index_maps() {
  const int64_t shapes[][2] = {{1, 1}, {2, 1}, {5, 3}, {3, 5}, {8, 8}, {7, 10}, {37, 64}};
  for (const auto& sh : shapes) {
    const int64_t n1 = sh[0], n2 = sh[1], P = xcorr_fft_length(n1, n2);
    std::vector<double> x((size_t)n1), y((size_t)n2);
    for (int64_t i = 0; i < n1; ++i) x[i] = (double)((i * 7 + 3) % 11) - 5.0;
    for (int64_t i = 0; i < n2; ++i) y[i] = (double)((i * 5 + 1) % 13) - 6.0;
    for (int32_t op = 0; op < 2; ++op) {
      // circular: correlate c[j] = sum_l x[l] y[(l - j) mod P], convolve c[k] = sum_l x[l] y[(k - l) mod P], y zero past n2
      std::vector<double> c((size_t)P, 0.0);
      for (int64_t j = 0; j < P; ++j)
        for (int64_t l = 0; l < n1; ++l) {
          const int64_t at = (((op == kXcCorrelate ? l - j : j - l) % P) + P) % P;
          if (at < n2) c[j] += x[l] * y[at];
        }
      for (int32_t mode = 0; mode < 3; ++mode) {
        const int64_t start = xcorr_out_start(n1, n2, mode), n_out = xcorr_out_length(n1, n2, mode), cs = xcorr_circ_start(n1, n2, op, mode, P);
        CHECK(start >= 0 && start + n_out <= n1 + n2 - 1 && cs >= 0 && cs < P, "window of (%lld, %lld) mode %d", (long long)n1, (long long)n2, mode);
        for (int64_t i = 0; i < n_out; ++i) {
          const int64_t k = start + i;
          double want = 0.0;   // the definition
          for (int64_t l = 0; l < n1; ++l) {
            const int64_t at = op == kXcCorrelate ? l - k + n2 - 1 : k - l;
            if (at >= 0 && at < n2) want += x[l] * y[at];
          }
          const int64_t j = xcorr_circ_index(cs, i, P);
          CHECK(j >= 0 && j < P && c[j] == want, "(%lld, %lld) op %d mode %d element %lld", (long long)n1, (long long)n2, op, mode, (long long)i);
          CHECK(xcorr_out_index(cs, j, P) == i, "the inverse map at %lld", (long long)i);
        }
      }
    }
  }
  // SciPy's windows and first lags on either side of n1 = n2
  CHECK(xcorr_out_length(3, 5, kXcValid) == 3 && xcorr_out_start(3, 5, kXcValid) == 2 && xcorr_first_lag(3, 5, kXcValid) == -2, "valid, n2 > n1");
  CHECK(xcorr_out_length(5, 3, kXcValid) == 3 && xcorr_out_start(5, 3, kXcValid) == 2 && xcorr_first_lag(5, 3, kXcValid) == 0, "valid, n1 > n2");
  CHECK(xcorr_first_lag(5, 3, kXcFull) == -2 && xcorr_first_lag(4, 3, kXcSame) == -1 && xcorr_first_lag(3, 4, kXcSame) == -1, "first lags");
  CHECK(xcorr_out_start(3, 4, kXcSame) == 1 && xcorr_out_start(4, 3, kXcSame) == 1, "same is centred on full");
}

static void test_mirror_and_scale() {
  for (int K : {1024, 2048}) {
    const int regs = K / 64;
    std::vector<int> seen((size_t)K, 0);
    for (int lane = 0; lane < 64; ++lane)
      for (int s = 0; s < regs; ++s) {
        const int k = czt_bin(lane, s), ml = xcorr_mirror_lane(lane), ms = xcorr_mirror_reg(lane, s, regs);
        CHECK(ml >= 0 && ml < 64 && ms >= 0 && ms < regs && czt_bin(ml, ms) == xcorr_mirror_bin(k, K), "mirror of bin %d at K = %d", k, K);
        CHECK(xcorr_mirror_lane(ml) == lane && xcorr_mirror_reg(ml, ms, regs) == s, "the mirror map is an involution at bin %d", k);
        CHECK((k + xcorr_mirror_bin(k, K)) % K == 0, "k + mirror = 0 mod K");
        ++seen[(size_t)czt_bin(ml, ms)];
      }
    for (int k = 0; k < K; ++k) CHECK(seen[(size_t)k] == 1, "bin %d is the mirror of %d bins", k, seen[(size_t)k]);
  }
  const float values[] = {1.0f, 0.5f, 0.75f, 0.99999994f, 3.0f, 1e4f, 1e-4f, 8192.0f, 1.17549435e-38f, 1e-40f, 1.4e-45f, 3.4028235e38f, -2.5f};
  for (float v : values) {
    uint32_t bits;
    std::memcpy(&bits, &v, sizeof bits);
    const int e = xcorr_scale_exponent(bits);
    const double scaled = std::ldexp(std::fabs((double)v), -e);
    CHECK(scaled >= 0.5 && scaled < 1.0, "the scale of %g brings it to %g", (double)v, scaled);
    CHECK((float)std::ldexp((double)std::ldexp(v, -e), e) == v, "the scale of %g is exact", (double)v);
  }
  CHECK(xcorr_scale_exponent(0u) == 0 && xcorr_scale_exponent(0x80000000u) == 0, "an all-zero row keeps scale 1");
  CHECK(xcorr_scale_exponent(0x7f800000u) == 0 && xcorr_scale_exponent(0x7fc00000u) == 0 && xcorr_scale_exponent(0xff800000u) == 0, "Inf and NaN keep scale 1");
}

static void test_slabs() {
  CHECK(xcorr_slab_rows(5, 1024, 2) == 2 && xcorr_slabs(5, 2) == 3, "a forced slab of 2 on batch 5");
  CHECK(xcorr_slab_rows(5, 1024, 0) == 5 && xcorr_slabs(5, 5) == 1, "a small batch is one slab");
  CHECK(xcorr_slab_rows(64, 131072, 0) == 64, "64 pairs of 2^17 points are one slab");
  CHECK(xcorr_slab_rows(100000, 1024, 0) == kXcorrSlabBytes / (4 * 1024 * 8), "the budget at P = 1024");
  CHECK(xcorr_slab_rows(7, (int64_t)1 << 30, 0) == 1 && xcorr_slab_rows(1, 1024, 9) == 1, "one pair at the least, the batch at the most");
  for (int64_t P = 1024; P <= ((int64_t)1 << 22); P <<= 1) {
    const int64_t rows = xcorr_slab_rows((int64_t)1 << 40, P, 0);
    CHECK(rows >= 1 && 4 * rows * P * 8 <= kXcorrSlabBytes, "the four temporaries at P = %lld", (long long)P);
  }
}

// the fused kernel's loads and stores, lane by lane: every sample below n read from an exactly sized buffer, every output element
// stored exactly once into one, for each K, op, mode and parity of the row start
static void test_lane_walk() {
  const int64_t shapes[][2] = {{1, 1}, {2, 1}, {5, 3}, {3, 5}, {600, 300}, {512, 513}, {513, 513}, {1024, 1025}, {1500, 549}, {1, 2048}, {2048, 1}};
  for (const auto& sh : shapes) {
    const int n1 = (int)sh[0], n2 = (int)sh[1], K = (int)xcorr_fft_length(n1, n2), NQ = K / 128;
    std::vector<float> a((size_t)n1, 1.0f);
    double sum = 0.0;
    for (int lane = 0; lane < 64; ++lane)
      for (int q = 0; q < NQ; ++q) {
        const int i0 = czt_slot_sample(lane, q), st = czt_pair_state(i0, n1);
        if (st >= 1) sum += a[(size_t)i0];
        if (st == 2) sum += a[(size_t)i0 + 1];
      }
    CHECK(sum == (double)n1, "every sample of a row of %d is loaded once", n1);
    for (int32_t op = 0; op < 2; ++op)
      for (int32_t mode = 0; mode < 3; ++mode) {
        const int64_t n_out = xcorr_out_length(n1, n2, mode), cs = xcorr_circ_start(n1, n2, op, mode, K);
        std::vector<int> out((size_t)n_out, 0);
        int pairs = 0;
        for (int lane = 0; lane < 64; ++lane)
          for (int q = 0; q < NQ; ++q) {
            const int64_t i0 = xcorr_out_index(cs, czt_slot_sample(lane, q), K), i1 = (i0 + 1) & (K - 1);
            const int st = xcorr_store_state(i0, i1, n_out);
            if (st & 4) {
              CHECK((st & 3) == 3 && i1 == i0 + 1, "a pair is two adjacent elements");
              ++pairs;
            }
            if (st & 1) ++out[(size_t)i0];
            if (st & 2) ++out[(size_t)i1];
          }
        for (int64_t i = 0; i < n_out; ++i) CHECK(out[(size_t)i] == 1, "(%d, %d) op %d mode %d: element %lld stored %d times", n1, n2, op, mode, (long long)i, out[(size_t)i]);
        CHECK(pairs >= (int)(n_out / 2) - 1, "(%d, %d) op %d mode %d: %d wide stores of %lld elements", n1, n2, op, mode, pairs, (long long)n_out);
      }
  }
  CHECK(czt_lds_bytes(1024) == 45568 && czt_lds_bytes(2048) == 53504 && czt_waves(1024) == 4 && czt_waves(2048) == 2, "czt.wave's budget");
}

int main() {
  test_checks_and_tier();
  test_index_maps();
  test_mirror_and_scale();
  test_slabs();
  test_lane_walk();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitized xcorr host side ok\n");
  return 0;
}
