// The host side of Filters.hilbert (csrc/hilbert_plan.hpp) in a stand-alone program for ASan / UBSan: the argument checks over a sweep
// of (length, n_fft, batch, batch_stride, kind) with the rejected ones, the multiplier rule against its definition and a naive DFT, the
// tier choice, and the row and lane arithmetic of the fused kernel walked lane by lane over heap buffers of exactly the size the C entry
// point is promised — a load or a store outside them is the sanitizer's to report.  Built and run by tests/test_hilbert_host.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hilbert_plan.hpp"

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

static void test_gain() {
  const int64_t lengths[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 1023, 1024, 2047, 2048};
  for (int64_t N : lengths) {
    int64_t sum = 0;
    for (int64_t k = 0; k < N; ++k) {
      const int g = hilbert_gain(k, N);
      int want = 0;
      if (k == 0) want = 1;
      else if (N % 2 == 0) want = k == N / 2 ? 1 : (k < N / 2 ? 2 : 0);
      else want = k < (N + 1) / 2 ? 2 : 0;
      CHECK(g == want, "gain(%lld, %lld) = %d, expected %d", (long long)k, (long long)N, g, want);
      sum += g;
    }
    CHECK(sum == N, "the gains of N = %lld sum to %lld", (long long)N, (long long)sum);
  }
  // in the kernel's layout the gain is a condition on the register index
  for (int P : {16, 32})
    for (int lane = 0; lane < 64; ++lane)
      for (int s = 0; s < P; ++s)
        CHECK(hilbert_wave_gain(lane, s, P) == hilbert_gain(lane + 64 * s, 64 * P), "wave gain lane %d register %d P %d", lane, s, P);
}

// a = IDFT(h DFT(x)) by the naive sums: a cosine over whole periods gives exp(i phase); Re a = x for any row
static void test_definition() {
  const double two_pi = 6.283185307179586476925286766559;
  for (int N : {1, 2, 3, 7, 8, 16, 33}) {
    std::vector<double> x(N);
    for (int n = 0; n < N; ++n) x[n] = std::cos(two_pi * n / N) + 0.25 * ((n * 37) % 11) - 1.0;
    std::vector<std::complex<double>> X(N), a(N);
    for (int k = 0; k < N; ++k) {
      std::complex<double> acc = 0.0;
      for (int n = 0; n < N; ++n) acc += x[n] * std::polar(1.0, -two_pi * (double)((int64_t)k * n % N) / N);
      X[k] = acc * (double)hilbert_gain(k, N);
    }
    for (int n = 0; n < N; ++n) {
      std::complex<double> acc = 0.0;
      for (int k = 0; k < N; ++k) acc += X[k] * std::polar(1.0, two_pi * (double)((int64_t)k * n % N) / N);
      a[n] = acc / (double)N;
      CHECK(std::fabs(a[n].real() - x[n]) <= 1e-12, "N = %d: Re a[%d] = %.17g, the sample is %.17g", N, n, a[n].real(), x[n]);
    }
  }
  const int N = 16;
  for (int n = 0; n < N; ++n) {   // x = cos(2 pi 3 n / N): a = exp(2 pi i 3 n / N)
    std::complex<double> acc = 0.0;
    for (int k = 0; k < N; ++k) {
      std::complex<double> Xk = 0.0;
      for (int m = 0; m < N; ++m) Xk += std::cos(two_pi * 3 * m / N) * std::polar(1.0, -two_pi * (double)(k * m % N) / N);
      acc += Xk * (double)hilbert_gain(k, N) * std::polar(1.0, two_pi * (double)(k * n % N) / N);
    }
    acc /= (double)N;
    CHECK(std::abs(acc - std::polar(1.0, two_pi * 3 * n / N)) <= 1e-12, "the analytic signal of a cosine at %d", n);
  }
}

static void test_checks_and_tier() {
  bool u = false;
  struct Case { int64_t length, batch, stride, n_fft; int32_t kind; const char* frag; bool unsupported; };
  const Case bad[] = {
      {0, 1, 8, 8, 0, "length must be >= 1", false},          {-3, 1, 8, 8, 0, "length must be >= 1", false},
      {8, 1, 8, 0, 0, "n_fft must be >= 1", false},           {8, 1, 8, -1, 0, "n_fft must be >= 1", false},
      {8, -1, 8, 8, 0, "batch must be >= 0", false},          {8, 2, 7, 8, 0, "batch_stride must be >= length", false},
      {8, 2, 8, 8, 3, "kind must be", false},                 {8, 2, 8, 8, -1, "kind must be", false},
      {8, 2, 8, (int64_t)1 << 31, 0, "below 2^31", true},     {(int64_t)1 << 59, 16, (int64_t)1 << 59, 8, 0, "too large", true},
      {8, (int64_t)1 << 30, 8, ((int64_t)1 << 31) - 1, 1, "too large", true},
  };
  for (const Case& c : bad) {
    const char* what = hilbert_check(c.length, c.batch, c.stride, c.n_fft, c.kind, &u);
    CHECK(what && std::strstr(what, c.frag) && u == c.unsupported, "check(%lld, %lld, %lld, %lld, %d) said %s", (long long)c.length,
          (long long)c.batch, (long long)c.stride, (long long)c.n_fft, c.kind, what ? what : "nothing");
  }
  CHECK(!hilbert_check(8, 0, 8, 8, 0, &u) && !u, "batch = 0 is valid");
  CHECK(!hilbert_check(1, 1, 1, 1, 2, &u), "a row of one sample");
  CHECK(!hilbert_check(2880000, 8, 2880000, 4194304, 0, &u), "8 x 60 s at 48 kHz");
  for (int64_t n : {1, 2, 512, 1000, 1023, 1025, 2047, 2049, 4096, 6000}) CHECK(hilbert_tier(n, false) == kHbGeneric, "tier of %lld", (long long)n);
  CHECK(hilbert_tier(1024, false) == kHbWave && hilbert_tier(2048, false) == kHbWave, "the fused lengths");
  CHECK(hilbert_tier(1024, true) == kHbGeneric && hilbert_tier(2048, true) == kHbGeneric, "the switch");
  CHECK(hilbert_used(1500, 1024) == 1024 && hilbert_used(1000, 1024) == 1000 && hilbert_used(1, 2048) == 1, "samples used");
  CHECK(hilbert_out_elem(kHbAnalytic) == 8 && hilbert_out_elem(kHbEnvelope) == 4 && hilbert_out_elem(kHbQuadrature) == 4, "element sizes");
  CHECK(hilbert_waves(1024) == 4 && hilbert_waves(2048) == 2, "waves per workgroup");
  CHECK(hilbert_lds_bytes(1024) == 45568 && hilbert_lds_bytes(2048) == 53504 && hilbert_lds_bytes(2048) <= 64 * 1024, "LDS per workgroup");
}

// the fused kernel's walk: workgroups of W waves over chunks of rows, every lane loading its pairs and storing its outputs, over buffers
// of exactly rows_bytes and batch * K elements
static void walk(int K, int64_t length, int64_t batch, int64_t stride, int32_t kind, int rows_per_wave) {
  bool u = false;
  CHECK(!hilbert_check(length, batch, stride, K, kind, &u), "walk arguments");
  const int W = hilbert_waves(K), NQ = K / 128;
  const int64_t chunk = (int64_t)W * rows_per_wave, blocks = hilbert_blocks(batch, chunk);
  const int n_used = (int)hilbert_used(length, K);
  std::vector<float> x((size_t)((batch - 1) * stride + length));
  for (size_t i = 0; i < x.size(); ++i) x[i] = (float)(i % 251) + 1.0f;
  const int per = kind == kHbAnalytic ? 2 : 1;
  std::vector<float> out((size_t)batch * K * per, 0.0f);
  std::vector<int> reads((size_t)batch * n_used, 0), writes((size_t)batch * K, 0);
  for (int64_t b = 0; b < blocks; ++b)
    for (int wave = 0; wave < W; ++wave) {
      int64_t r_end = (b + 1) * chunk;
      if (r_end > batch) r_end = batch;
      for (int64_t r = b * chunk + wave; r < r_end; r += W)
        for (int lane = 0; lane < 64; ++lane)
          for (int q = 0; q < NQ; ++q) {
            const int i0 = hilbert_slot_sample(lane, q), st = hilbert_pair_state(i0, n_used);
            const float* row = x.data() + (size_t)r * stride;
            float v0 = 0.0f, v1 = 0.0f;
            if (st >= 1) { v0 = row[i0]; ++reads[(size_t)r * n_used + i0]; }
            if (st == 2) { v1 = row[i0 + 1]; ++reads[(size_t)r * n_used + i0 + 1]; }
            float* o = out.data() + ((size_t)r * K + i0) * per;
            for (int e = 0; e < 2 * per; ++e) o[e] = e < per ? v0 : v1;
            ++writes[(size_t)r * K + i0];
            ++writes[(size_t)r * K + i0 + 1];
          }
    }
  for (size_t i = 0; i < reads.size(); ++i) CHECK(reads[i] == 1, "K %d L %lld: sample %zu read %d times", K, (long long)length, i, reads[i]);
  for (size_t i = 0; i < writes.size(); ++i) CHECK(writes[i] == 1, "K %d L %lld: output %zu written %d times", K, (long long)length, i, writes[i]);
  for (int64_t r = 0; r < batch; ++r)
    for (int i = 0; i < K; ++i) {
      const float want = i < n_used ? x[(size_t)r * stride + i] : 0.0f;
      CHECK(out[((size_t)r * K + i) * per] == want, "K %d row %lld index %d: the walk carried %g, the row holds %g", K, (long long)r, i,
            out[((size_t)r * K + i) * per], want);
    }
}

int main() {
  test_gain();
  test_definition();
  test_checks_and_tier();
  for (int K : {1024, 2048})
    for (int64_t length : {(int64_t)1, (int64_t)2, (int64_t)127, (int64_t)1000, (int64_t)K - 1, (int64_t)K, (int64_t)K + 1, (int64_t)3000})
      for (int64_t batch : {1, 2, 3, 65})
        for (int64_t gap : {0, 5})
          for (int32_t kind : {kHbAnalytic, kHbEnvelope, kHbQuadrature})
            for (int rpw : {1, 4}) walk(K, length, batch, length + gap, kind, rpw);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitized hilbert host side ok\n");
  return 0;
}
