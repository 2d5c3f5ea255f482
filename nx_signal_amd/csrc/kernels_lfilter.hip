// Filters.lfilter / filtfilt: a transfer function (b, a) of order n <= 16 in transposed direct form II over real f32 rows, scipy.signal's
// definition; include/nxsig.h states it, DESIGN.md section 3.18 the design.  Coefficients, states and the recurrence are double.
//
//   lfilter.scan     the n states of the direct form are the linear system z[m + 1] = A z[m] + B x[m] with A a dense companion matrix:
//                    the recurrence scan of recurrence_scan.hpp, whose kernels and driver this file instantiates with the direct form's
//                    step and with dense NP x NP products.  The tables are built on the host (lfilter_plan.hpp), which also decides
//                    whether a filter may use them: a direct form with clustered poles has powers too badly conditioned for this
//                    algebra although the plain recurrence is fine (the conditioning guard).  Chunk and tile depend on the order only.
//   lfilter.generic  one lane per row, the plain recurrence: rows of at most one chunk, every filter the guard keeps off the scan, and
//                    NXSIG_DISABLE_LFILTER_SCAN
// b and a are filled up with zeros to the order 1 / 2 / 4 / 8 / 16 a kernel is instantiated for; a padded state stays an exact zero.
#include "nxsig_internal.h"
#include "recurrence_scan.hpp"

namespace nxsig {
namespace {

// what the family tells the driver of recurrence_scan.hpp
struct LfFamily {
  using Launch = LfLaunch;
  static constexpr const char* kTooManyTiles = "lfilter: 2^31 or more tiles in one call";
  static constexpr const char* kTooManyBlocks = "filtfilt: 2^31 or more tiles in one call";
  static int states(const Launch& a) { return a.cf.n; }   // a gain has no state
  static int32_t chunk(const Launch& a) { return lf_chunk(a.cf.n); }
  static int64_t tiles(const Launch& a) { return lf_tiles(a.n, a.cf.n); }
  static void note(bool scan) {
    if (scan) dispatch_note("lfilter.scan");
    else dispatch_note("lfilter.generic");
  }
  static int launch(Ctx* c, const Launch& a) { return launch_lfilter(c, a); }
};

template <int N> struct Lf : LfFamily {
  static constexpr int NP = N;
  struct Coefs { double b[NP + 1], a[NP + 1]; };   // divided by a[0]; a[0] == 1 is not read

  static Coefs fill(const Launch& a) {
    Coefs cf;
    for (int k = 0; k <= NP; ++k) { cf.b[k] = a.cf.b[k]; cf.a[k] = a.cf.a[k]; }
    return cf;
  }

  // one sample: y = b0 x + z0;  z[i] = z[i + 1] + b[i + 1] x - a[i + 1] y;  z[NP - 1] = b[NP] x - a[NP] y
  static __device__ __forceinline__ double step(const Coefs& cf, double (&z)[NP], double x) {
    const double y = __builtin_fma(cf.b[0], x, z[0]);
#pragma unroll
    for (int i = 0; i < NP - 1; ++i) z[i] = __builtin_fma(cf.b[i + 1], x, __builtin_fma(-cf.a[i + 1], y, z[i + 1]));
    z[NP - 1] = __builtin_fma(cf.b[NP], x, -cf.a[NP] * y);
    return y;
  }

  // v += M w for a dense M, ascending columns
  static __device__ __forceinline__ void matvec_add(double (&v)[NP], const double* __restrict__ M, const double (&w)[NP]) {
#pragma unroll
    for (int r = 0; r < NP; ++r) {
      double acc = v[r];
#pragma unroll
      for (int c = 0; c < NP; ++c) acc = __builtin_fma(M[r * NP + c], w[c], acc);
      v[r] = acc;
    }
  }

  // The tables of a filter are built once per context and (R, b, a): the memo keeps the device pointers and the guard's verdict beside
  // the key's content, so a later call neither forms the powers again nor asks for a table.  Dropped together with the table cache
  // (DeviceGuard, api.cpp).  *scan_ok false: the conditioning guard keeps the filter off the scan (no table was uploaded)
  static int tables(Ctx* c, const Launch& a, int64_t R, const void** mcd, const void** mtd, bool* scan_ok) {
    const LfCoefs& cf = a.cf;
    const int n = cf.n;
    std::vector<uint64_t> want((size_t)4 + 2 * (n + 1));
    want[2] = ((uint64_t)R << 8) | (uint64_t)n;
    std::memcpy(want.data() + 4, cf.b, (size_t)(n + 1) * sizeof(double));
    std::memcpy(want.data() + 4 + (n + 1), cf.a, (size_t)(n + 1) * sizeof(double));
    const uint64_t key = fnv1a(0x11f17e00ull ^ ((uint64_t)NP << 40) ^ (uint64_t)R, want.data() + 4, (size_t)2 * (n + 1) * sizeof(double));
    auto hit = c->memo.find(key);
    if (hit != c->memo.end() && hit->second.size() == want.size() && hit->second[2] == want[2] && std::equal(want.begin() + 4, want.end(), hit->second.begin() + 4)) {
      *mcd = reinterpret_cast<const void*>((uintptr_t)hit->second[0]);
      *mtd = reinterpret_cast<const void*>((uintptr_t)hit->second[1]);
      *scan_ok = hit->second[3] != 0;
      return NXSIG_OK;
    }
    const LfTables t = lf_tables(cf, R);
    *mcd = *mtd = nullptr;
    *scan_ok = t.scan_ok;
    if (t.scan_ok) {
      int rc;
      if ((rc = ctx_table(c, 0x11f17e43ull ^ ((uint64_t)NP << 32), t.mc.data(), t.mc.size() * sizeof(double), mcd))) return rc;
      if ((rc = ctx_table(c, 0x11f17f43ull ^ ((uint64_t)NP << 32), t.mt.data(), t.mt.size() * sizeof(double), mtd))) return rc;
    }
    want[0] = (uint64_t)(uintptr_t)*mcd;
    want[1] = (uint64_t)(uintptr_t)*mtd;
    want[3] = t.scan_ok ? 1 : 0;
    c->memo[key] = want;
    return NXSIG_OK;
  }

  // filtfilt's zi is a function of (b, a): one cached table per filter
  static int zi_table(Ctx* c, const std::vector<double>& padded, const void** d) {
    return ctx_table(c, 0x11f17a49ull ^ ((uint64_t)NP << 32), padded.data(), padded.size() * sizeof(double), d);
  }
};

}  // namespace

int launch_lfilter(Ctx* c, const LfLaunch& a) {
  // a row of one chunk has nothing to run side by side: the plain recurrence (a rule of the row length and the order only)
  const bool scan = !tune(c, kT_DISABLE_LFILTER_SCAN, 0) && a.n > lf_chunk(a.cf.n);
  return rscan::run_padded<Lf>(c, a, lf_padded_order(a.cf.n), scan);
}

int launch_filtfilt(Ctx* c, const float* x, int64_t n, int64_t x_stride, int32_t batch, const LfCoefs& cf, int32_t padtype, int64_t edge, float* y) {
  double zi[kLfMaxOrder];
  if (!lf_zi(cf, zi)) return set_error(NXSIG_ERR_INVALID_ARG, "filtfilt: singular matrix");
  LfLaunch a{};
  a.cf = cf; a.zi_host = zi;
  return rscan::forward_backward<LfFamily>(c, x, n, x_stride, batch, padtype, edge, y, a);
}

}  // namespace nxsig
