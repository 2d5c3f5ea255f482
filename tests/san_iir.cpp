// TEST INFRASTRUCTURE: AddressSanitizer / UndefinedBehaviorSanitizer run of the host side of Filters.sosfilt / sosfiltfilt that needs no
// GPU (nx_signal_amd/csrc/iir_plan.hpp): the argument checks, the chunk / tile geometry, sosfilt_zi, the padding rule, and the matrices
// of the scan.  Built and run by tests/test_iir_host.py with g++ -fsanitize=address,undefined -fno-sanitize-recover.  A^C is held to C
// steps of the recurrence, and the whole scheme of kernels_iir.hip — pass 1, the scan over the 64 lanes of a tile, the carry over the
// tiles of a row with R tiles per lane, pass 2 — is played on the host with the very matrices the kernels read (padded to the
// instantiated section count) and held to the plain recurrence, through std::vector::at so that an index outside a table aborts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "iir_plan.hpp"

using namespace nxsig;
typedef std::vector<double> vec;

static int fail(const char* what, long a, long b, double v) {
  std::printf("FAILED %s (%ld, %ld, %g)\n", what, a, b, v);
  return 1;
}

// v += M w, M np x np row-major, the columns the kernels visit (0 .. r | 1)
static void matvec_add(vec& v, const vec& M, size_t off, const vec& w, int np) {
  for (int r = 0; r < np; ++r)
    for (int c = 0; c <= (r | 1); ++c) v.at(r) += M.at(off + (size_t)r * np + c) * w.at(c);
}

// the scan of the kernels over `lanes` state vectors
static void scan(std::vector<vec>& v, const vec& M, int np) {
  for (int k = 0; k < kIirLevels; ++k) {
    const std::vector<vec> w = v;
    for (int lane = 1 << k; lane < (int)v.size(); ++lane) matvec_add(v.at(lane), M, (size_t)k * np * np, w.at(lane - (1 << k)), np);
  }
}

static double rnd(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(int64_t)(s >> 11) / (double)(1ull << 52) - 1.0;
}

// the scheme on a row of n samples against the recurrence; returns the largest error over the largest output magnitude
static double play(const double* sos, int S, int64_t n, const double* zi, double* zf_err) {
  const int np = 2 * iir_padded_sections(S), n2 = 2 * S, C = iir_chunk(S), T = iir_tile(S);
  const int64_t tiles = iir_tiles(n, S), R = iir_tiles_per_lane(tiles);
  uint64_t seed = 12345 + (uint64_t)n;
  vec x((size_t)n), ref((size_t)n), got((size_t)n);
  for (auto& v : x) v = (double)(float)(rnd(seed) + 0.5);
  vec s(n2, 0.0);
  if (zi) for (int k = 0; k < n2; ++k) s[k] = zi[k];
  for (int64_t i = 0; i < n; ++i) ref[i] = iir_step(sos, S, s.data(), x[i]);
  const vec zf_ref = s;

  const vec A = iir_state_matrix(sos, S);
  const vec mc = iir_scan_matrices(A, n2, np, (uint64_t)C, 0);
  const vec mt = iir_scan_matrices(A, n2, np, (uint64_t)T * (uint64_t)R, (uint64_t)T);
  auto run_chunk = [&](int64_t l0, vec& st, bool write) {
    for (int64_t i = l0; i < l0 + C && i < n; ++i) {
      const double y = iir_step(sos, S, st.data(), x[i]);
      if (write) got.at((size_t)i) = y;
    }
  };
  // pass 1
  std::vector<std::vector<vec>> P((size_t)tiles);
  for (int64_t t = 0; t < tiles; ++t) {
    P[t].assign(kIirLanes, vec(np, 0.0));
    for (int lane = 0; lane < kIirLanes; ++lane) run_chunk((t * kIirLanes + lane) * C, P[t][lane], false);
    scan(P[t], mc, np);
  }
  // carry
  std::vector<vec> acc(kIirLanes, vec(np, 0.0)), start((size_t)tiles, vec(np, 0.0));
  const size_t single = (size_t)kIirLevels * np * np;
  for (int lane = 0; lane < kIirLanes; ++lane)
    for (int64_t t = lane * R; t < (lane + 1) * R && t < tiles; ++t) {
      vec z = P[t][kIirLanes - 1];
      matvec_add(z, mt, single, acc[lane], np);
      acc[lane] = z;
    }
  vec s0(np, 0.0);
  if (zi) for (int k = 0; k < n2; ++k) s0[k] = zi[k];
  matvec_add(acc[0], mt, 0, s0, np);
  scan(acc, mt, np);
  for (int lane = 0; lane < kIirLanes; ++lane) {
    vec st = lane == 0 ? s0 : acc[lane - 1];
    for (int64_t t = lane * R; t < (lane + 1) * R && t < tiles; ++t) {
      start.at((size_t)t) = st;
      vec z = P[t][kIirLanes - 1];
      matvec_add(z, mt, single, st, np);
      st = z;
    }
  }
  // pass 2
  vec zf(np, 0.0);
  for (int64_t t = 0; t < tiles; ++t) {
    std::vector<vec> u(kIirLanes, vec(np, 0.0));
    u[0] = start[t];
    scan(u, mc, np);
    for (int lane = 0; lane < kIirLanes; ++lane) {
      vec st = u[lane];
      if (lane > 0) for (int k = 0; k < np; ++k) st[k] += P[t][lane - 1][k];
      const int64_t l0 = (t * kIirLanes + lane) * C;
      run_chunk(l0, st, true);
      if (l0 < n && l0 + C >= n) zf = st;
    }
  }
  double big = 0.0, err = 0.0, zbig = 0.0, zerr = 0.0;
  for (int64_t i = 0; i < n; ++i) { big = std::fmax(big, std::fabs(ref[i])); err = std::fmax(err, std::fabs(ref[i] - got[i])); }
  for (int k = 0; k < n2; ++k) { zbig = std::fmax(zbig, std::fabs(zf_ref[k])); zerr = std::fmax(zerr, std::fabs(zf_ref[k] - zf[k])); }
  *zf_err = zbig > 0 ? zerr / zbig : zerr;
  return big > 0 ? err / big : err;
}

int main() {
  int bad = 0;
  // ---- geometry: functions of n_sections only
  for (int s = -1; s <= 18; ++s) {
    const int32_t c = iir_chunk(s), t = iir_tile(s);
    if (s < 1 || s > 16) { if (c != 0 || t != 0) bad += fail("geometry outside", s, c, t); continue; }
    if (c < kIirSub || c % kIirSub || t != c * kIirLanes || iir_padded_sections(s) < s || iir_padded_sections(s) > 16) bad += fail("geometry", s, c, t);
  }
  if (iir_tiles(1, 1) != 1 || iir_tiles(2048, 1) != 1 || iir_tiles(2049, 2) != 2 || iir_tiles(4096, 3) != 1 || iir_tiles_per_lane(64) != 1 ||
      iir_tiles_per_lane(65) != 2 || iir_tiles_per_lane(1) != 1)
    bad += fail("tiles", 0, 0, 0);
  // ---- argument checks
  const double two[12] = {0.02, 0.04, 0.02, 1.0, -1.2, 0.4, 1.0, -0.5, 0.25, 1.0, -0.9, 0.5};
  double bad_a0[12], nan_b[12];
  for (int i = 0; i < 12; ++i) { bad_a0[i] = two[i]; nan_b[i] = two[i]; }
  bad_a0[9] = 2.0; nan_b[1] = NAN;
  if (iir_check_sos(two, 2) || !iir_check_sos(two, 0) || !iir_check_sos(two, -3) || !iir_check_sos(bad_a0, 2) || !iir_check_sos(nan_b, 2) ||
      iir_check_sos(bad_a0, 1))
    bad += fail("check_sos", 0, 0, 0);
  struct { int64_t L; int32_t b; int64_t bs; int32_t zr; bool zi; int32_t dir; bool ok; } cases[] = {
      {40, 2, 40, 2, true, 0, true},  {40, 2, 40, 1, true, 1, true},  {40, 2, 40, 7, false, 0, true}, {0, 2, 40, 1, false, 0, false},
      {40, 0, 40, 1, false, 0, false}, {40, 2, 39, 1, false, 0, false}, {40, 2, 40, 3, true, 0, false}, {40, 2, 40, 1, false, 2, false},
      {40, 2, 40, 1, false, -1, false}, {INT64_MAX, INT32_MAX, INT64_MAX, 1, true, 1, true}};
  for (const auto& c : cases)
    if ((iir_check_args(c.L, c.b, c.bs, c.zr, c.zi, c.dir) == nullptr) != c.ok) bad += fail("check_args", (long)c.L, c.b, c.dir);
  // ---- sosfiltfilt's edge: scipy's default 3 * (2 S + 1 - min(#b2 == 0, #a2 == 0))
  const double hp1[6] = {0.99, -0.99, 0.0, 1.0, -0.98, 0.0};
  if (iir_default_padlen(two, 2) != 15 || iir_default_padlen(hp1, 1) != 6 || iir_edge(two, 2, 1, -1, 16) != 15 || iir_edge(two, 2, 1, -1, 15) != -2 ||
      iir_edge(two, 2, 0, 99, 1) != 0 || iir_edge(two, 2, 4, 0, 10) != -1 || iir_edge(two, 2, -1, 0, 10) != -1 || iir_edge(two, 2, 3, 0, 1) != 0 ||
      iir_edge(two, 2, 2, 9, 10) != 9 || iir_edge(two, 2, 2, 10, 10) != -2 || iir_edge(two, 2, 2, INT64_MAX, INT64_MAX) != -2)
    bad += fail("edge", 0, 0, 0);
  // ---- sosfilt_zi: the state a unit step settles in (one more step leaves it unchanged and the output is the DC gain)
  {
    double zi[4];
    if (!iir_sosfilt_zi(two, 2, zi)) bad += fail("zi", 0, 0, 0);
    double s[4] = {zi[0], zi[1], zi[2], zi[3]};
    const double y = iir_step(two, 2, s, 1.0);
    const double dc = (0.08 / 0.2) * (0.75 / 0.6);
    if (std::fabs(y - dc) > 1e-14) bad += fail("zi output", 0, 0, y);
    for (int k = 0; k < 4; ++k) if (std::fabs(s[k] - zi[k]) > 1e-14) bad += fail("zi settled", k, 0, s[k] - zi[k]);
    const double integ[6] = {1.0, 0.0, 0.0, 1.0, -1.0, 0.0};
    if (iir_sosfilt_zi(integ, 1, zi)) bad += fail("zi of a pole at 1", 0, 0, 0);
  }
  // ---- cascades: 1, 2, 3, 5 and 16 sections, poles inside, on (integrator) and outside (radius 1.001) the unit circle
  std::vector<vec> filters;
  filters.push_back(vec(two, two + 6));
  filters.push_back(vec(two, two + 12));
  filters.push_back({1.0, 0.0, 0.0, 1.0, -1.0, 0.0});
  // butter(4, 20 Hz, "hp") at 48 kHz: two pole pairs at radius 0.999 within 0.15 degrees of z = 1, A nearly defective — the cascade
  // whose powers need the extended precision of iir_matpow_wide (in double its states came out 3e-8 off)
  filters.push_back({0.996585268514311, -1.993170537028622, 0.996585268514311, 1.0, -1.9951674183225134, 0.9951742556729883, 1.0, -2.0, 1.0, 1.0, -1.9979914349390582, 0.9979982819673131});
  filters.push_back({1.0, 0.0, 0.0, 1.0, -2.0 * 1.001 * std::cos(0.3), 1.001 * 1.001});
  for (int S : {3, 5, 16}) {
    vec f;
    for (int k = 0; k < S; ++k) {
      const double r = 0.90 + 0.0995 * k / S, th = 0.05 + 0.17 * k;
      const double sec[6] = {0.3, 0.1 * (k % 3), -0.2, 1.0, -2.0 * r * std::cos(th), r * r};
      f.insert(f.end(), sec, sec + 6);
    }
    filters.push_back(f);
  }
  long plays = 0;
  double worst = 0.0;
  for (const vec& f : filters) {
    const int S = (int)(f.size() / 6), n2 = 2 * S, C = iir_chunk(S), T = iir_tile(S);
    // A^C against C steps of the recurrence from every unit state and from a mixed one
    const vec A = iir_state_matrix(f.data(), S);
    const vec AC = iir_matpow(A, n2, (uint64_t)C);
    for (int c = 0; c <= n2; ++c) {
      vec s(n2, 0.0);
      if (c < n2) s[c] = 1.0; else for (int k = 0; k < n2; ++k) s[k] = 0.25 * (k + 1) * (k % 2 ? -1 : 1);
      const vec s_in = s;
      for (int i = 0; i < C; ++i) iir_step(f.data(), S, s.data(), 0.0);
      double big = 0.0;
      for (int r = 0; r < n2; ++r) big = std::fmax(big, std::fabs(s[r]));
      for (int r = 0; r < n2; ++r) {
        double v = 0.0;
        for (int k = 0; k < n2; ++k) v += AC[(size_t)r * n2 + k] * s_in[k];
        if (std::fabs(v - s[r]) > 1e-11 * std::fmax(big, 1e-300)) bad += fail("A^C", S, r, v - s[r]);
      }
    }
    // block lower triangular: what the kernels skip is zero
    for (int r = 0; r < n2; ++r)
      for (int c = (r | 1) + 1; c < n2; ++c) if (AC[(size_t)r * n2 + c] != 0.0) bad += fail("triangle", S, r, AC[(size_t)r * n2 + c]);
    // the whole scheme: one chunk, a tile seam, several tiles, more than 64 tiles (R = 2)
    vec zi((size_t)n2);
    for (int k = 0; k < n2; ++k) zi[k] = 0.1 * (k + 1);
    const bool unstable = S == 1 && f[5] > 1.0;
    for (int64_t n : {(int64_t)1, (int64_t)C - 1, (int64_t)C + 1, (int64_t)T, (int64_t)T + 1, (int64_t)3 * T + C + 1, (int64_t)65 * T + 3}) {
      if (unstable && n > 3000) n = 3000;
      for (int with_zi = 0; with_zi <= 1; ++with_zi) {
        double zf_err = 0.0;
        const double e = play(f.data(), S, n, with_zi ? zi.data() : nullptr, &zf_err);
        ++plays;
        // round-off of the scheme against round-off of the recurrence: at most 1.7e-11 on these cascades; the bound sits a decade above
        // that, three decades below the 6e-8 of the final rounding to f32
        worst = std::fmax(worst, std::fmax(e, zf_err));
        if (!(e <= 1e-10) || !(zf_err <= 1e-10)) bad += fail("scheme", S, (long)n, e > zf_err ? e : zf_err);
      }
    }
  }
  if (bad) return 1;
  std::printf("sanitized iir host side ok: %ld plays, worst %.2e\n", plays, worst);
  return 0;
}
