// TEST INFRASTRUCTURE: AddressSanitizer / UndefinedBehaviorSanitizer run of the host side of Filters.lfilter / filtfilt that needs no GPU
// (nx_signal_amd/csrc/lfilter_plan.hpp): the argument checks, the normalisation, the chunk / tile geometry, lfilter_zi, the padding
// rule, the tables of the scan and the conditioning guard.  Built and run by tests/test_lfilter_host.py with
// g++ -fsanitize=address,undefined -fno-sanitize-recover.  The whole scheme of kernels_lfilter.hip (pass 1, the scan over the 64 lanes
// of a tile, the carry over the tiles of a row with R tiles per lane, pass 2) is played on the host with the very tables the kernels
// read, every product dense over the padded order, over exactly sized heap buffers read through std::vector::at.  The catalogue of
// the design is held to the recurrence in long double: at most 1e-7 of the row maximum for every filter the guard
// lets onto the scan; every filter it rejects is printed with the figure the scan would have had without the guard.  Random filters
// with their poles in one cluster follow (300 in the test run, `san_lfilter --sweep N` for more): the same bound for whatever passes.
// `san_lfilter --figures` prints one line per filter and row length (profiles/lfilter/accuracy.txt).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lfilter_plan.hpp"

using namespace nxsig;
typedef std::vector<double> vec;

static int fail(const char* what, long a, long b, double v) {
  std::printf("FAILED %s (%ld, %ld, %g)\n", what, a, b, v);
  return 1;
}

// v += M w, M np x np row-major at `off`, every column (the kernels' products are dense)
static void matvec_add(vec& v, const vec& M, size_t off, const vec& w, int np) {
  for (int r = 0; r < np; ++r) {
    double acc = v.at(r);
    for (int c = 0; c < np; ++c) acc += M.at(off + (size_t)r * np + c) * w.at(c);
    v.at(r) = acc;
  }
}

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
// about normal: the sum of twelve uniforms, rounded to f32 as a sample is
static double noise(uint64_t& s) {
  double v = 0.0;
  for (int k = 0; k < 12; ++k) v += rnd(s);
  return (double)(float)v;
}

// the step in the padded order np, as a lane runs it (coefficients past the order are zero)
static double step_padded(const LfCoefs& cf, int np, vec& z, double x) {
  const double y = z.at(0) + cf.b[0] * x;
  for (int i = 0; i < np - 1; ++i) z.at(i) = z.at(i + 1) + x * cf.b[i + 1] - y * cf.a[i + 1];
  z.at(np - 1) = x * cf.b[np] - y * cf.a[np];
  return y;
}

struct Figures { double plain, scheme, zf; };

// the scheme on a row of n samples against the recurrence in long double; errors over the largest reference magnitude
static Figures play(const LfCoefs& cf, const LfTables& tb, int64_t n, int64_t R, const double* zi) {
  const int order = cf.n, np = lf_padded_order(order), C = lf_chunk(order);
  const int64_t tiles = lf_tiles(n, order);
  uint64_t seed = 12345 + (uint64_t)n;
  vec x((size_t)n), got((size_t)n), plain((size_t)n);
  std::vector<long double> ref((size_t)n), zl((size_t)(order ? order : 1), 0.0L);
  for (auto& v : x) v = noise(seed);
  vec zd((size_t)(order ? order : 1), 0.0);
  if (zi) for (int k = 0; k < order; ++k) { zd[k] = zi[k]; zl[k] = zi[k]; }
  for (int64_t i = 0; i < n; ++i) {
    plain[i] = lf_step(cf, zd.data(), x[i]);
    const long double xv = x[i];
    if (order == 0) { ref[i] = (long double)cf.b[0] * xv; continue; }
    const long double y = zl[0] + (long double)cf.b[0] * xv;
    for (int k = 0; k < order - 1; ++k) zl[k] = zl[k + 1] + xv * (long double)cf.b[k + 1] - y * (long double)cf.a[k + 1];
    zl[order - 1] = xv * (long double)cf.b[order] - y * (long double)cf.a[order];
    ref[i] = y;
  }

  auto run_chunk = [&](int64_t l0, vec& st, bool write) {
    for (int64_t i = l0; i < l0 + C && i < n; ++i) {
      const double y = step_padded(cf, np, st, x.at((size_t)i));
      if (write) got.at((size_t)i) = y;
    }
  };
  // pass 1
  std::vector<std::vector<vec>> P((size_t)tiles);
  for (int64_t t = 0; t < tiles; ++t) {
    P[t].assign(kIirLanes, vec(np, 0.0));
    for (int lane = 0; lane < kIirLanes; ++lane) run_chunk((t * kIirLanes + lane) * C, P[t][lane], false);
    scan(P[t], tb.mc, np);
  }
  // carry
  std::vector<vec> acc(kIirLanes, vec(np, 0.0)), start((size_t)tiles, vec(np, 0.0));
  const size_t single = (size_t)kIirLevels * np * np;
  for (int lane = 0; lane < kIirLanes; ++lane)
    for (int64_t t = lane * R; t < (lane + 1) * R && t < tiles; ++t) {
      vec z = P[t][kIirLanes - 1];
      matvec_add(z, tb.mt, single, acc[lane], np);
      acc[lane] = z;
    }
  vec s0(np, 0.0);
  if (zi) for (int k = 0; k < order; ++k) s0[k] = zi[k];
  matvec_add(acc[0], tb.mt, 0, s0, np);
  scan(acc, tb.mt, np);
  for (int lane = 0; lane < kIirLanes; ++lane) {
    vec st = lane == 0 ? s0 : acc[lane - 1];
    for (int64_t t = lane * R; t < (lane + 1) * R && t < tiles; ++t) {
      start.at((size_t)t) = st;
      vec z = P[t][kIirLanes - 1];
      matvec_add(z, tb.mt, single, st, np);
      st = z;
    }
  }
  // pass 2
  vec zf(np, 0.0);
  for (int64_t t = 0; t < tiles; ++t) {
    std::vector<vec> u(kIirLanes, vec(np, 0.0));
    u[0] = start[t];
    scan(u, tb.mc, np);
    for (int lane = 0; lane < kIirLanes; ++lane) {
      vec st = u[lane];
      if (lane > 0) for (int k = 0; k < np; ++k) st[k] += P[t][lane - 1][k];
      const int64_t l0 = (t * kIirLanes + lane) * C;
      run_chunk(l0, st, true);
      if (l0 < n && l0 + C >= n) zf = st;
    }
  }
  long double big = 0.0L, e_plain = 0.0L, e_scheme = 0.0L, zbig = 0.0L, zerr = 0.0L;
  for (int64_t i = 0; i < n; ++i) {
    big = fmaxl(big, fabsl(ref[i]));
    e_plain = fmaxl(e_plain, fabsl(ref[i] - (long double)plain[i]));
    e_scheme = fmaxl(e_scheme, fabsl(ref[i] - (long double)got[i]));
  }
  for (int k = 0; k < order; ++k) { zbig = fmaxl(zbig, fabsl(zl[k])); zerr = fmaxl(zerr, fabsl(zl[k] - (long double)zf[k])); }
  for (int k = order; k < np; ++k) if (zf[k] != 0.0 && std::isfinite(zf[k])) zerr = INFINITY;   // a padded state is an exact zero
  Figures f;
  const long double den = big > 0 ? big : 1.0L;
  f.plain = (double)(e_plain / den);
  f.scheme = (double)(e_scheme / den);
  f.zf = (double)(zbig > 0 ? zerr / zbig : zerr);
  if (!(f.plain == f.plain)) f.plain = INFINITY;     // the reference itself overflowed: an unstable filter
  if (!(f.scheme == f.scheme)) f.scheme = INFINITY;
  return f;
}

// the catalogue of DESIGN.md section 3.18: scipy.signal 1.15.3 designs, printed with 17 digits (fs = 48 kHz where a corner is in Hz)
struct Entry { const char* name; vec b, a; };
static const std::vector<Entry>& catalogue() {
  static const std::vector<Entry> c = {
  {"butter(2, .2)", {0.067455273889071896, 0.13491054777814379, 0.067455273889071896}, {1, -1.1429805025399011, 0.41280159809618877}},
  {"butter(4, .1)", {0.00041659920440659937, 0.0016663968176263975, 0.0024995952264395961, 0.0016663968176263975, 0.00041659920440659937}, {1, -3.1806385488747191, 3.8611943489942133, -2.1121553551109691, 0.43826514226197977}},
  {"butter(2, 20 Hz, hp)", {0.99815051119045184, -1.9963010223809037, 0.99815051119045184}, {1, -1.9962976017691221, 0.99630444299268572}},
  {"butter(4, 20 Hz, hp)", {0.99658526851431095, -3.9863410740572438, 5.9795116110858659, -3.9863410740572438, 0.99658526851431095}, {1, -3.9931588532615718, 5.9794999507181563, -3.9795232948295114, 0.99318219741974201}},
  {"cheby1(8, 1, 100 Hz)", {5.138894007889979e-20, 4.1111152063119832e-19, 1.438890322209194e-18, 2.877780644418388e-18, 3.5972258055229854e-18, 2.877780644418388e-18, 1.438890322209194e-18, 4.1111152063119832e-19, 5.138894007889979e-20}, {1, -7.9876173613549568, 27.913739808769432, -55.7424704661764, 69.572862901187264, -55.574935470619906, 27.746201123415037, -7.9158124319692869, 0.98803189674882108}},
  {"butter(4, [.2, .4], bp)", {0.0048243433577162325, 0, -0.01929737343086493, 0, 0.028946060146297393, 0, -0.01929737343086493, 0, 0.0048243433577162325}, {1, -3.936575530223053, 8.2603942952917517, -11.217425904032236, 10.78363101479793, -7.3914428343704923, 3.5765049292123559, -1.115046647904617, 0.18737949236818485}},
  {"ellip(6, .5, 60, .3)", {0.0074347762152226059, 0.0047698622413100741, 0.015217180132555934, 0.010430936873814438, 0.015217180132555937, 0.0047698622413100775, 0.0074347762152226059}, {1, -3.6611964294152006, 6.6064875704306791, -7.1015437011665217, 4.7551380975297866, -1.8693143711175719, 0.3395711694627615}},
  {"butter(12, .3)", {6.8612578966895157e-06, 8.2335094760274189e-05, 0.00045284302118150802, 0.0015094767372716934, 0.0033963226588613104, 0.0054341162541780962, 0.0063398022965411123, 0.0054341162541780962, 0.0033963226588613104, 0.0015094767372716934, 0.00045284302118150802, 8.2335094760274189e-05, 6.8612578966895157e-06}, {1, -4.7896857933357726, 11.645464058343629, -18.346021383577899, 20.563662020431018, -17.111889121343857, 10.770286559285944, -5.1410704971286219, 1.8402453442508557, -0.48028403826894994, 0.086540721680223157, -0.0096462998080420106, 0.00050214181631578429}},
  {"butter(16, .4)", {5.2825969859266053e-06, 8.4521551774825686e-05, 0.00063391163831119266, 0.0029582543121188989, 0.0096143265143864218, 0.023074383634527414, 0.042303036663300257, 0.060432909519000363, 0.067987023208875411, 0.060432909519000363, 0.042303036663300257, 0.023074383634527414, 0.0096143265143864218, 0.0029582543121188989, 0.00063391163831119266, 8.4521551774825686e-05, 5.2825969859266053e-06}, {1, -3.1952148891208214, 6.7795359678336533, -9.8717285428619128, 11.21693765282199, -10.067329148660052, 7.3805958118944828, -4.4312806134879805, 2.1970521063935542, -0.89478877596276285, 0.29769318876396828, -0.079648630305528115, 0.016769218846106781, -0.0026767575643227397, 0.00030503958227448785, -2.2120096272790855e-05, 7.6799330947323474e-07}},
  {"cheby2(16, 40, .5)", {0.068410040566209945, 0.45338186567853844, 1.7290662744575243, 4.714468169411032, 10.064680184752428, 17.595975955176176, 25.850784160664116, 32.392521451652669, 34.893546721004583, 32.392521451652733, 25.850784160664105, 17.595975955176151, 10.064680184752421, 4.7144681694110329, 1.7290662744575254, 0.45338186567853872, 0.068410040566209959}, {1, 3.2557026304013972, 8.5474161255569516, 15.883190443164324, 24.623055254033474, 31.612921742968375, 34.817462595378174, 32.980000418806029, 27.061878416953846, 19.19565463832252, 11.713022267906675, 6.0797490603280009, 2.6354314324225685, 0.92538935882714302, 0.24977333926707468, 0.04679526762978152, 0.0046799337558146937}},
  {"integrator", {1}, {1, -1}},
  {"pre-emphasis .97", {1, -0.96999999999999997}, {1}},
  {"gain 0.5", {0.5}, {1}},
  {"butter(3, 20 Hz, hp)", {0.99738542933367291, -2.9921562880010186, 2.9921562880010186, -0.99738542933367291}, {1, -2.9947640137392946, 2.9895417262829724, -0.99477769464711463}},
  {"butter(3, 40 Hz, hp)", {0.99477769018464135, -2.9843330705539239, 2.9843330705539239, -0.99477769018464135}, {1, -2.9895280364500225, 2.9791108321380184, -0.98958265288908975}},
  {"butter(3, 100 Hz, hp)", {0.98699523941366962, -2.9609857182410089, 2.9609857182410089, -0.98699523941366962}, {1, -2.9738202481010347, 2.947982064583154, -0.97415960262517109}},
  {"butter(4, 40 Hz, hp)", {0.99318219059987389, -3.9727287623994956, 5.9590931435992438, -3.9727287623994956, 0.99318219059987389}, {1, -3.9863177122115898, 5.9590466614474762, -3.959139812214155, 0.98641086372476461}},
  {"butter(4, 60 Hz, hp)", {0.9897907197127751, -3.9591628788511004, 5.9387443182766511, -3.9591628788511004, 0.9897907197127751}, {1, -3.9794765825381813, 5.9386400907558059, -3.938849173280885, 0.9796856688295339}},
  {"butter(4, 100 Hz, hp)", {0.98304241398428849, -3.932169655937154, 5.8982544839057311, -3.932169655937154, 0.98304241398428849}, {1, -3.9657943800700517, 5.8979669386140863, -3.8985449173724191, 0.96637238769205691}},
  {"butter(5, 100 Hz, hp)", {0.97904252295968175, -4.8952126147984085, 9.790425229596817, -9.790425229596817, 4.8952126147984085, -0.97904252295968175}, {1, -4.9576400574733732, 9.831456026088091, -9.7485160479301349, 4.8332243414549669, -0.95852426176325956}},
  {"butter(3, .9)", {0.72944072263908211, 2.1883221679172462, 2.1883221679172462, 0.72944072263908211}, {1, 2.3740947437093518, 1.9293556690912148, 0.53207536831209157}},
  {"butter(5, .5)", {0.052786404500042045, 0.26393202250021019, 0.52786404500042039, 0.52786404500042039, 0.26393202250021019, 0.052786404500042045}, {1, -4.163336342344337e-16, 0.63343685400050476, -1.318605337420283e-16, 0.055728090000841203, -3.0935304318658431e-18}},
  {"butter(9, .3)", {0.00013337394932935224, 0.0012003655439641703, 0.004801462175856681, 0.011203411743665589, 0.016805117615498383, 0.016805117615498383, 0.011203411743665589, 0.004801462175856681, 0.0012003655439641703, 0.00013337394932935224}, {1, -3.5863092537427552, 6.558719601082033, -7.5519676307257395, 5.9363214384279752, -3.2605664369891509, 1.2421309203192643, -0.31457688584795945, 0.047855829996854525, -0.0033201204638935366}},
  {"a[0] = 2", {2.0, 1.0}, {2.0, -1.0, 0.5}},
  // poles clustered at a moderate radius: powers that grow to 1e5 inside a chunk and are gone by A^64 (no table entry is large)
  {"bessel(14, .2)", {6.3461308004556637e-09, 8.8845831206379296e-08, 5.7749790284146539e-07, 2.3099916113658616e-06, 6.3524769312561191e-06, 1.2704953862512238e-05, 1.9057430793768358e-05, 2.1779920907163839e-05, 1.9057430793768358e-05, 1.2704953862512238e-05, 6.3524769312561191e-06, 2.3099916113658616e-06, 5.7749790284146539e-07, 8.8845831206379296e-08, 6.3461308004556637e-09}, {1, -7.989558901646201, 30.288002145360437, -72.07620339279903, 120.0931179087751, -148.00371149521965, 138.96109417057065, -100.86835798708518, 56.827695790957634, -24.707178318756078, 8.1540182692861194, -1.9794299460617588, 0.33391026105533916, -0.035015815200706776, 0.0017212857703513486}},
  {"15 clustered poles", {0.27273658715551841, 0.36518353827535599, 0.27183723603060861, 0.15745595425437364, -0.29681868138516748, 0.11776707958842714, 0.20520791347557832}, {1, 8.1296365891807376, 30.986199505642588, 73.448516914606799, 121.07920036793605, 147.03267080639773, 135.87156890890205, 97.291640308314896, 54.426514308647022, 23.786663775577544, 8.055427746020472, 2.0759357166416503, 0.39409114091060349, 0.052029641131200004, 0.0042719092382498183, 0.00016444422801214139}},
  {"pole pair at radius 1.001", {1.0}, {1.0, -2.0 * 1.001 * 0.95533648912560598, 1.001 * 1.001}},
  };
  return c;
}

// a random filter with its poles in one cluster: order 6 .. 16, centre radius 0.5 .. 0.95 at any angle, the poles within a few
// per cent of it; up to seven numerator coefficients.  The denominator is multiplied out in long double and rounded once
static void clustered(uint64_t& seed, vec& b, vec& a) {
  auto u = [&]() { return 0.5 * (rnd(seed) + 1.0); };
  const int order = 6 + (int)(u() * 10.999);
  const double r0 = 0.5 + 0.45 * u(), th0 = 3.141592653589793 * u(), spread = 0.002 + 0.1 * u();
  std::vector<long double> p(1, 1.0L);
  auto times = [&](const std::vector<long double>& q) {
    std::vector<long double> out(p.size() + q.size() - 1, 0.0L);
    for (size_t i = 0; i < p.size(); ++i)
      for (size_t j = 0; j < q.size(); ++j) out[i + j] += p[i] * q[j];
    p = out;
  };
  int left = order;
  while (left >= 2) {
    const long double r = std::fmin(0.97, r0 * (1.0 + spread * rnd(seed))), th = th0 + spread * rnd(seed);
    times({1.0L, -2.0L * r * cosl(th), r * r});
    left -= 2;
  }
  if (left) times({1.0L, (long double)-std::fmin(0.97, r0 * (1.0 + spread * rnd(seed)))});
  a.assign(p.begin(), p.end());
  b.assign((size_t)(1 + (int)(u() * 6.999)), 0.0);
  for (auto& v : b) v = 0.4 * rnd(seed);
  if (b[0] == 0.0) b[0] = 0.25;
}

int main(int argc, char** argv) {
  const bool figures = argc > 1 && !std::strcmp(argv[1], "--figures");
  int bad = 0;
  // ---- geometry: functions of the order only
  for (int n = -2; n <= 18; ++n) {
    const int32_t c = lf_chunk(n), t = lf_tile(n);
    if (n < 0 || n > 16) { if (c != 0 || t != 0) bad += fail("geometry outside", n, c, t); continue; }
    const int np = lf_padded_order(n);
    if (c < kIirSub || c % kIirSub || t != c * kIirLanes || np < n || np > 16 || (np & (np - 1))) bad += fail("geometry", n, c, t);
  }
  if (lf_tiles(1, 0) != 1 || lf_tiles(2048, 4) != 1 || lf_tiles(2049, 4) != 2 || lf_tiles(4096, 5) != 1 || lf_tiles(4097, 16) != 2) bad += fail("tiles", 0, 0, 0);
  // ---- argument checks and the normalisation
  {
    const double b2[2] = {2.0, 1.0}, a3[3] = {2.0, -1.0, 0.5}, a0[2] = {0.0, 1.0}, nanv[2] = {1.0, NAN};
    vec longa(18, 0.1);
    longa[0] = 1.0;
    bool un = true;
    if (lf_check_ba(b2, 2, a3, 3, &un) || un) bad += fail("check valid", 0, 0, 0);
    if (!lf_check_ba(b2, 0, a3, 3, &un) || un || !lf_check_ba(b2, 2, a3, 0, &un) || !lf_check_ba(b2, 2, a0, 2, &un) || un || !lf_check_ba(nanv, 2, a3, 3, &un) ||
        !lf_check_ba(b2, 2, nanv, 2, &un) || un)
      bad += fail("check invalid", 0, 0, 0);
    if (!lf_check_ba(b2, 2, longa.data(), 18, &un) || !un || !lf_check_ba(longa.data(), 18, b2, 1, &un) || !un || lf_check_ba(longa.data(), 17, b2, 1, &un))
      bad += fail("check order", 0, 0, 0);
    const LfCoefs cf = lf_normalise(b2, 2, a3, 3);
    if (cf.n != 2 || cf.b[0] != 1.0 || cf.b[1] != 0.5 || cf.b[2] != 0.0 || cf.a[0] != 1.0 || cf.a[1] != -0.5 || cf.a[2] != 0.25 || cf.a[16] != 0.0)
      bad += fail("normalise", cf.n, 0, cf.b[1]);
    // lfilter_zi: the state a unit step settles in
    double zi[2];
    if (!lf_zi(cf, zi)) bad += fail("zi", 0, 0, 0);
    double z[2] = {zi[0], zi[1]};
    const double y = lf_step(cf, z, 1.0), dc = 1.5 / 0.75;
    if (std::fabs(y - dc) > 1e-14 || std::fabs(z[0] - zi[0]) > 1e-14 || std::fabs(z[1] - zi[1]) > 1e-14) bad += fail("zi settled", 0, 0, y - dc);
    const double one[1] = {1.0}, integ[2] = {1.0, -1.0};
    if (lf_zi(lf_normalise(one, 1, integ, 2), zi)) bad += fail("zi of a pole at 1", 0, 0, 0);
    if (!lf_zi(lf_normalise(one, 1, one, 1), zi)) bad += fail("zi of a gain", 0, 0, 0);
  }
  // ---- filtfilt's edge: scipy's default 3 max(na, nb)
  if (lf_default_padlen(3, 5) != 15 || lf_default_padlen(2, 1) != 6 || lf_edge(3, 5, 1, -1, 16) != 15 || lf_edge(3, 5, 1, -1, 15) != -2 || lf_edge(3, 5, 0, 99, 1) != 0 ||
      lf_edge(3, 5, 4, 0, 10) != -1 || lf_edge(3, 5, -1, 0, 10) != -1 || lf_edge(3, 5, 3, 0, 1) != 0 || lf_edge(3, 5, 2, 9, 10) != 9 || lf_edge(3, 5, 2, 10, 10) != -2 ||
      lf_edge(3, 5, 2, INT64_MAX, INT64_MAX) != -2)
    bad += fail("edge", 0, 0, 0);

  // ---- the catalogue: the scheme with and without zi on 6 000 samples (one tile and a seam), a row that crosses the carry's second
  // level (R = 2) and the short lengths around a chunk and a tile
  long plays = 0;
  double worst_pass = 0.0;
  int passed = 0, rejected = 0;
  for (const Entry& e : catalogue()) {
    bool un = false;
    if (lf_check_ba(e.b.data(), (int32_t)e.b.size(), e.a.data(), (int32_t)e.a.size(), &un)) { bad += fail("catalogue entry", 0, 0, 0); continue; }
    const LfCoefs cf = lf_normalise(e.b.data(), (int32_t)e.b.size(), e.a.data(), (int32_t)e.a.size());
    const int order = cf.n, C = lf_chunk(order), T = lf_tile(order);
    const bool growing = !std::strcmp(e.name, "cheby1(8, 1, 100 Hz)") || !std::strcmp(e.name, "pole pair at radius 1.001");
    vec zi((size_t)(order ? order : 1));
    for (int k = 0; k < order; ++k) zi[k] = 0.1 * (k + 1);
    bool ok_everywhere = true;
    double kappa_max = 0.0, worst = 0.0, worst_plain = 0.0;
    for (int64_t n : {(int64_t)1, (int64_t)C - 1, (int64_t)C + 1, (int64_t)T, (int64_t)T + 1, (int64_t)6000, (int64_t)65 * T + 3}) {
      if (growing && n > 6000) continue;   // the reference itself leaves the range of a double
      const int64_t R = iir_tiles_per_lane(lf_tiles(n, order));
      const LfTables tb = lf_tables(cf, R);
      if ((int)tb.mc.size() != 7 * lf_padded_order(order) * lf_padded_order(order) || tb.mt.size() != tb.mc.size()) bad += fail("table size", order, 0, 0);
      ok_everywhere = ok_everywhere && tb.scan_ok;
      kappa_max = std::fmax(kappa_max, tb.kappa);
      bool finite = true;
      for (double v : tb.mt) finite = finite && std::isfinite(v);
      if (!finite) { worst = INFINITY; continue; }   // nothing to play: the guard must have refused it
      for (int with_zi = 0; with_zi <= 1; ++with_zi) {
        const Figures f = play(cf, tb, n, R, with_zi ? zi.data() : nullptr);
        ++plays;
        worst = std::fmax(worst, std::fmax(f.scheme, f.zf));
        worst_plain = std::fmax(worst_plain, f.plain);
        if (figures)
          std::printf("%-26s order %2d n %7ld zi %d R %ld kappa %.2e guard %s plain %.1e scan %.1e zf %.1e\n", e.name, order, (long)n, with_zi, (long)R, tb.kappa,
                      tb.scan_ok ? "scan" : "generic", f.plain, f.scheme, f.zf);
      }
    }
    if (ok_everywhere) {
      ++passed;
      worst_pass = std::fmax(worst_pass, worst);
      std::printf("scan     %-26s order %2d kappa %.2e plain %.1e scan %.1e\n", e.name, order, kappa_max, worst_plain, worst);
      if (!(worst <= 1e-7)) bad += fail("a filter the guard lets onto the scan misses 1e-7", order, 0, worst);
    } else {
      ++rejected;
      std::printf("generic  %-26s order %2d kappa %.2e plain %.1e unguarded scan %.1e\n", e.name, order, kappa_max, worst_plain, worst);
    }
  }
  if (passed < 10 || rejected < 2) bad += fail("the guard's split of the catalogue", passed, rejected, 0);

  // ---- random clustered-pole filters on 6 000 samples: whatever the guard lets onto the scan is within 1e-7 there as well, and the
  // table's A^C of such a filter, read back through at(), agrees with C steps of the recurrence (the guard's own second condition)
  {
    const long count = argc > 2 && !std::strcmp(argv[1], "--sweep") ? std::atol(argv[2]) : 300;
    uint64_t seed = 20261021;
    long on_scan = 0, beyond = 0;
    double worst_sweep = 0.0, kappa_of_worst = 0.0, worst_rejected_plain = 0.0;
    for (long i = 0; i < count; ++i) {
      vec b, a;
      clustered(seed, b, a);
      const LfCoefs cf = lf_normalise(b.data(), (int32_t)b.size(), a.data(), (int32_t)a.size());
      const int64_t n = 6000, R = iir_tiles_per_lane(lf_tiles(n, cf.n));
      const LfTables tb = lf_tables(cf, R);
      bool finite = true;
      for (double v : tb.mt) finite = finite && std::isfinite(v);
      if (!finite) { if (tb.scan_ok) bad += fail("a non-finite table on the scan", i, 0, 0); continue; }
      const Figures f = play(cf, tb, n, R, nullptr);
      ++plays;
      if (figures || argc > 2)
        std::printf("sweep %4ld order %2d growth %.2e kappa %.2e gap %.1e guard %s plain %.1e scan %.1e\n", i, cf.n, tb.growth, tb.kappa, tb.table_gap,
                    tb.scan_ok ? "scan" : "generic", f.plain, f.scheme);
      if (!tb.scan_ok) { if (f.scheme > 1e-7) { ++beyond; worst_rejected_plain = std::fmax(worst_rejected_plain, f.plain); } continue; }
      ++on_scan;
      if (f.scheme > worst_sweep) { worst_sweep = f.scheme; kappa_of_worst = tb.kappa; }
      if (!(f.scheme <= 1e-7) || !(f.zf <= 1e-7)) bad += fail("a clustered filter on the scan misses 1e-7", i, cf.n, f.scheme);
      const int np = lf_padded_order(cf.n), C = lf_chunk(cf.n);
      for (int c = 0; c < cf.n; ++c) {
        vec z((size_t)cf.n, 0.0);
        z.at(c) = 1.0;
        for (int k = 0; k < C; ++k) lf_step(cf, z.data(), 0.0);
        for (int r = 0; r < cf.n; ++r)
          if (std::fabs(z.at(r) - tb.mc.at((size_t)r * np + c)) > kLfTableGapMax * tb.growth) bad += fail("A^C of the table", i, r, z.at(r));
      }
    }
    std::printf("sweep: %ld clustered filters, %ld on the scan (worst %.2e at kappa %.2e), %ld of the others beyond 1e-7 without the guard (plain <= %.1e)\n", count,
                on_scan, worst_sweep, kappa_of_worst, beyond, worst_rejected_plain);
    if (on_scan < count / 20) bad += fail("the sweep hardly reaches the scan", on_scan, count, 0);
  }
  if (bad) return 1;
  std::printf("sanitized lfilter host side ok: %ld plays, %d filters on the scan (worst %.2e), %d on the plain recurrence\n", plays, passed, worst_pass, rejected);
  return 0;
}
