// Filters.sosfilt / sosfiltfilt: cascades of biquads in transposed direct form II over real f32 rows, scipy.signal's definition;
// include/nxsig.h states it, DESIGN.md section 3.13 the design.  Coefficients, states and the recurrence are double.
//
//   sosfilt.scan     a cascade of S sections is the linear system s[n + 1] = A s[n] + B x[n] with 2 S states: the recurrence scan of
//                    recurrence_scan.hpp, whose kernels and driver this file instantiates with the cascade's step and with products
//                    that know A^k to be block lower triangular.  The matrices are built on the host (iir_plan.hpp); chunk and tile
//                    depend on S only.
//   sosfilt.generic  one lane per row, the plain recurrence: rows of at most one chunk, and NXSIG_DISABLE_SOSFILT_SCAN
// The cascade is filled up to 1 / 2 / 4 / 8 / 16 sections with identity sections, whose state stays zero.
#include "nxsig_internal.h"
#include "recurrence_scan.hpp"

namespace nxsig {
namespace {

// what the family tells the driver of recurrence_scan.hpp
struct SosFamily {
  using Launch = IirLaunch;
  static constexpr const char* kTooManyTiles = "sosfilt: 2^31 or more tiles in one call";
  static constexpr const char* kTooManyBlocks = "sosfiltfilt: 2^31 or more tiles in one call";
  static int states(const Launch& a) { return 2 * a.n_sections; }
  static int32_t chunk(const Launch& a) { return iir_chunk(a.n_sections); }
  static int64_t tiles(const Launch& a) { return iir_tiles(a.n, a.n_sections); }
  static void note(bool scan) {
    if (scan) dispatch_note("sosfilt.scan");
    else dispatch_note("sosfilt.generic");
  }
  static int launch(Ctx* c, const Launch& a) { return launch_sosfilt(c, a); }
};

template <int SP> struct Sos : SosFamily {
  static constexpr int NP = 2 * SP;
  struct Coefs { double c[SP][5]; };   // b0 b1 b2 a1 a2 per section (a0 == 1)

  static Coefs fill(const Launch& a) {
    Coefs cf;
    for (int k = 0; k < SP; ++k) {
      const double ident[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
      const double* q = k < a.n_sections ? a.sos_host + 6 * k : ident;
      cf.c[k][0] = q[0]; cf.c[k][1] = q[1]; cf.c[k][2] = q[2]; cf.c[k][3] = q[4]; cf.c[k][4] = q[5];
    }
    return cf;
  }

  // one sample through the cascade: scipy's recurrence, y = b0 x + z0; z0 = b1 x - a1 y + z1; z1 = b2 x - a2 y
  static __device__ __forceinline__ double step(const Coefs& cf, double (&s)[NP], double x) {
#pragma unroll
    for (int k = 0; k < SP; ++k) {
      const double y = __builtin_fma(cf.c[k][0], x, s[2 * k]);
      s[2 * k] = __builtin_fma(cf.c[k][1], x, __builtin_fma(-cf.c[k][3], y, s[2 * k + 1]));
      s[2 * k + 1] = __builtin_fma(cf.c[k][2], x, -cf.c[k][4] * y);
      x = y;
    }
    return x;
  }

  // v += M w for a block lower triangular M (row r sees columns 0 .. r | 1), ascending columns
  static __device__ __forceinline__ void matvec_add(double (&v)[NP], const double* __restrict__ M, const double (&w)[NP]) {
#pragma unroll
    for (int r = 0; r < NP; ++r) {
      double acc = v[r];
#pragma unroll
      for (int c = 0; c <= (r | 1); ++c) acc = __builtin_fma(M[r * NP + c], w[c], acc);
      v[r] = acc;
    }
  }

  // The matrices of a cascade are built once per context and (R, sos): the memo keeps the device pointers beside the key's content,
  // so a later call neither forms the powers again (milliseconds of extended-precision products at 16 sections) nor hashes them.
  // Dropped together with the table cache (DeviceGuard, api.cpp).  Every cascade may run the scan
  static int tables(Ctx* c, const Launch& a, int64_t R, const void** mcd, const void** mtd, bool*) {
    const int S = a.n_sections, n2 = 2 * S;
    const uint64_t key = fnv1a(0x11525300ull ^ ((uint64_t)NP << 40) ^ (uint64_t)R, a.sos_host, (size_t)S * 6 * sizeof(double));
    std::vector<uint64_t> want((size_t)3 + 6 * S);
    want[2] = ((uint64_t)R << 8) | (uint64_t)S;
    std::memcpy(want.data() + 3, a.sos_host, (size_t)S * 6 * sizeof(double));
    auto hit = c->memo.find(key);
    if (hit != c->memo.end() && hit->second.size() == want.size() && std::equal(want.begin() + 2, want.end(), hit->second.begin() + 2)) {
      *mcd = reinterpret_cast<const void*>((uintptr_t)hit->second[0]);
      *mtd = reinterpret_cast<const void*>((uintptr_t)hit->second[1]);
      return NXSIG_OK;
    }
    const std::vector<double> A = iir_state_matrix(a.sos_host, S);
    const std::vector<double> mc = iir_scan_matrices(A, n2, NP, (uint64_t)iir_chunk(S), 0);
    const std::vector<double> mt = iir_scan_matrices(A, n2, NP, (uint64_t)iir_tile(S) * (uint64_t)R, (uint64_t)iir_tile(S));
    int rc;
    if ((rc = ctx_table(c, 0x11525343ull ^ ((uint64_t)NP << 32), mc.data(), mc.size() * sizeof(double), mcd))) return rc;
    if ((rc = ctx_table(c, 0x11525443ull ^ ((uint64_t)NP << 32), mt.data(), mt.size() * sizeof(double), mtd))) return rc;
    want[0] = (uint64_t)(uintptr_t)*mcd;
    want[1] = (uint64_t)(uintptr_t)*mtd;
    c->memo[key] = want;
    return NXSIG_OK;
  }

  // sosfiltfilt's zi is a function of sos: one cached table per cascade
  static int zi_table(Ctx* c, const std::vector<double>& padded, const void** d) {
    return ctx_table(c, 0x11522149ull ^ ((uint64_t)NP << 32), padded.data(), padded.size() * sizeof(double), d);
  }
};

}  // namespace

int launch_sosfilt(Ctx* c, const IirLaunch& a) {
  // a row of one chunk has nothing to run side by side: the plain recurrence (a rule of the row length and n_sections only)
  const bool scan = !tune(c, kT_DISABLE_SOSFILT_SCAN, 0) && a.n > iir_chunk(a.n_sections);
  return rscan::run_padded<Sos>(c, a, iir_padded_sections(a.n_sections), scan);
}

int launch_sosfiltfilt(Ctx* c, const float* x, int64_t n, int64_t x_stride, int32_t batch, const double* sos_host, int32_t n_sections,
                       int32_t padtype, int64_t edge, float* y) {
  std::vector<double> zi((size_t)2 * n_sections);
  if (!iir_sosfilt_zi(sos_host, n_sections, zi.data())) return set_error(NXSIG_ERR_INVALID_ARG, "sosfiltfilt: singular matrix");
  IirLaunch a{};
  a.sos_host = sos_host; a.n_sections = n_sections; a.zi_host = zi.data();
  return rscan::forward_backward<SosFamily>(c, x, n, x_stride, batch, padtype, edge, y, a);
}

}  // namespace nxsig
