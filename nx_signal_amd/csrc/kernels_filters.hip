// NxSignal.Filters.median/2 and wiener/2 (lib/nx_signal/filters.ex:17-55, :81-110, :281-303): sliding-window median and the
// local-statistics Wiener filter over n-D tensors, f32 or f64.
//
// median — three tiers that return the same bits (selection is exact, the even-window mean is formed one way):
//   median.rows     window along the last axis only, k <= 31: one row segment + its forward halo in LDS, two neighbouring outputs per
//                   thread share one sorting network over their k - 1 common samples
//   median.plane    window over the last two axes only, k_h, k_w <= 7: the same on a 2-D tile (k_h (k_w - 1) common samples, one
//                   sorted column of k_h per output, the order statistic read off the two sorted lists with min / max)
//   median.generic  any rank <= 8, any window: rank selection by bisection over the keys (32 / 64 counting passes), no arrays
// Values are compared through order-preserving integer keys: NaN is mapped to the canonical +NaN above +Inf (np.sort's order —
// fminf / fmaxf would drop it) and -0.0 to +0.0.
//
// wiener — S1 / S2 of the window in f64, accumulated from 0.0 in the window's row-major order (the reference's correlate), then
// the formula; no FMA contraction anywhere in this file (the reference rounds every product and sum on its own):
//   wiener.plane    window on the last two axes: an f64 LDS tile with the :same halo
//   wiener.generic  any rank <= 8
// noise: nil runs pass 1 (l_var partial sums per workgroup, in a fixed order), one workgroup that reduces them in a fixed order, and
// pass 2 (S1 / S2 recomputed, cheaper than keeping 16 B per element).  No atomics: the result does not change from run to run.
#pragma clang fp contract(off)

#include <utility>

#include "nxsig_internal.h"

namespace nxsig {
namespace {

constexpr int kMedianRowsMaxK = 31, kMedianPlaneMaxK = 7;   // the tiers' window bounds (larger windows run median.generic)

// ---------------------------------------------------------------------------------------------------------------------------------
// order-preserving keys
template <typename T> struct Keys;
template <> struct Keys<float> {
  using K = uint32_t;
  static constexpr int kBits = 32;
  __device__ static __forceinline__ K key(float v) {
    uint32_t u = __float_as_uint(v);
    if (v != v) u = 0x7fc00000u;          // every NaN -> +NaN, above +Inf
    else if (v == 0.0f) u = 0u;           // -0.0 == +0.0
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
  }
  __device__ static __forceinline__ float val(K k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
  // Nx.median of an even window: (a + b) / 2 in the input's type
  __device__ static __forceinline__ float mean2(K a, K b) { return (val(a) + val(b)) / 2.0f; }
  __device__ static __forceinline__ float out(K a) { return val(a); }
};
template <> struct Keys<double> {
  using K = uint64_t;
  static constexpr int kBits = 64;
  __device__ static __forceinline__ K key(double v) {
    uint64_t u = (uint64_t)__double_as_longlong(v);
    if (v != v) u = 0x7ff8000000000000ull;
    else if (v == 0.0) u = 0ull;
    return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
  }
  __device__ static __forceinline__ double val(K k) { return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull))); }
  __device__ static __forceinline__ float mean2(K a, K b) { return (float)((val(a) + val(b)) / 2.0); }
  __device__ static __forceinline__ float out(K a) { return (float)val(a); }
};

template <typename K> __device__ __forceinline__ void cmpx(K& a, K& b) {
  const K lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

constexpr int pow2_at_least(int n) { return n <= 1 ? 1 : 2 * pow2_at_least((n + 1) / 2); }

// Batcher's odd-even merge sort of a[0, P), P a power of two; entries past the live ones hold the largest key, so the comparators
// that touch them fold away at compile time
template <int P, typename K> __device__ __forceinline__ void sort_net(K (&a)[P]) {
#pragma unroll
  for (int p = 1; p < P; p <<= 1)
#pragma unroll
    for (int k = p; k >= 1; k >>= 1)
#pragma unroll
      for (int j = k % p; j + k < P; j += 2 * k)
#pragma unroll
        for (int i = 0; i < k; ++i)
          if (i + j + k < P && (i + j) / (2 * p) == (i + j + k) / (2 * p)) cmpx(a[i + j], a[i + j + k]);
}

// r-th smallest (0-based) of the union of two sorted lists S[0, M) and C[0, H): min over the splits j of max(S[r - j], C[j - 1])
template <int M, int H, int PS, int PC, typename K> __device__ __forceinline__ K kth_of_union(const K (&S)[PS], const K (&C)[PC], int r_) {
  const int k = r_ + 1;
  K best = ~(K)0;
#pragma unroll
  for (int j = 0; j <= H; ++j) {
    const int i = k - j;
    if (i < 0 || i > M) continue;
    const K a = i > 0 ? S[i - 1] : (K)0, b = j > 0 ? C[j - 1] : (K)0;
    const K m = a > b ? a : b;
    best = best < m ? best : m;
  }
  return best;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// median.rows / median.plane: tensor viewed as [B][H][W], window KH x KW on the last two axes (KH = 1: rows).  A workgroup of BX x BY
// threads owns a tile of BY rows x 2 BX columns of outputs; each thread two horizontally neighbouring outputs.
template <int KH, int KW> struct TileShape {
  static constexpr int BX = KH == 1 ? 256 : 64, BY = KH == 1 ? 1 : 4;
  static constexpr int TW = 2 * BX, TH = BY, LW = TW + KW - 1, LH = TH + KH - 1;
};

template <typename T, int KH, int KW>
__global__ __launch_bounds__(256) void k_median_tile(const T* __restrict__ x, float* __restrict__ out, int64_t H, int64_t W, int64_t tiles_w,
                                                     int64_t tiles_h) {
  using KT = Keys<T>;
  using K = typename KT::K;
  using S = TileShape<KH, KW>;
  __shared__ K tile[S::LH * S::LW];
  const int64_t blk = blockIdx.x;
  const int64_t tw = blk % tiles_w, th = (blk / tiles_w) % tiles_h, b = blk / (tiles_w * tiles_h);
  const int64_t r0 = th * S::TH, c0 = tw * S::TW;
  const int64_t rs = r0 < H - KH ? r0 : H - KH, cs = c0 < W - KW ? c0 : W - KW;   // clamped window starts (Nx.slice)
  const T* xb = x + b * H * W;
  for (int e = threadIdx.x; e < S::LH * S::LW; e += 256) {
    const int lr = e / S::LW, lc = e % S::LW;
    const int64_t gr = rs + lr, gc = cs + lc;
    tile[e] = (gr < H && gc < W) ? KT::key(xb[gr * W + gc]) : ~(K)0;
  }
  __syncthreads();
  const int tx = threadIdx.x % S::BX, ty = threadIdx.x / S::BX;
  const int64_t i = r0 + ty, j0 = c0 + 2 * tx;
  if (i >= H || j0 >= W) return;
  const int wr = (int)((i < H - KH ? i : H - KH) - rs);
  const int wc0 = (int)((j0 < W - KW ? j0 : W - KW) - cs);
  const int wc1 = (int)((j0 + 1 < W - KW ? j0 + 1 : W - KW) - cs);
  constexpr int M = KH * (KW - 1), PM = pow2_at_least(M), PC = pow2_at_least(KH);
  K com[PM], ca[PC], cb[PC];
#pragma unroll
  for (int q = 0; q < PM; ++q) com[q] = ~(K)0;
#pragma unroll
  for (int q = 0; q < PC; ++q) ca[q] = cb[q] = ~(K)0;
  const int cx = wc0 + (wc1 - wc0) * KW;   // the second output's own column (its window is the first one's when clamped)
#pragma unroll
  for (int dr = 0; dr < KH; ++dr) {
    const K* row = tile + (wr + dr) * S::LW;
#pragma unroll
    for (int dc = 1; dc < KW; ++dc) com[dr * (KW - 1) + dc - 1] = row[wc0 + dc];
    ca[dr] = row[wc0];
    cb[dr] = row[cx];
  }
  if (M > 1) sort_net<PM>(com);
  if (KH > 1) {
    sort_net<PC>(ca);
    sort_net<PC>(cb);
  }
  constexpr int N = KH * KW;
  float o0, o1;
  if (N % 2) {
    o0 = KT::out(kth_of_union<M, KH>(com, ca, N / 2));
    o1 = KT::out(kth_of_union<M, KH>(com, cb, N / 2));
  } else {
    o0 = KT::mean2(kth_of_union<M, KH>(com, ca, N / 2 - 1), kth_of_union<M, KH>(com, ca, N / 2));
    o1 = KT::mean2(kth_of_union<M, KH>(com, cb, N / 2 - 1), kth_of_union<M, KH>(com, cb, N / 2));
  }
  float* ob = out + (b * H + i) * W;
  ob[j0] = o0;
  if (j0 + 1 < W) ob[j0 + 1] = o1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// n-D geometry of the generic kernels.  Only the window axes (k > 1) are walked; `wsize` = their product.
struct NdGeom {
  int32_t rank, nwin;
  int64_t total, wsize;
  int64_t n[8], stride[8];
  int64_t wk[8], wstride[8], wlo[8];   // per window axis (row-major order): length, input stride, low padding (wiener)
  int32_t wax[8];                      // which tensor axis
  int64_t k[8];                        // window length per tensor axis (median start clamp)
};

// input offset of window element w (flat, last window axis fastest) relative to the window's first element
__device__ __forceinline__ int64_t win_off(const NdGeom& g, int64_t w) {
  int64_t off = 0;
  for (int a = g.nwin - 1; a >= 0; --a) {
    const int64_t q = w % g.wk[a];
    w /= g.wk[a];
    off += q * g.wstride[a];
  }
  return off;
}

template <typename T>
__global__ __launch_bounds__(256) void k_median_generic(const T* __restrict__ x, float* __restrict__ out, NdGeom g) {
  using KT = Keys<T>;
  using K = typename KT::K;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < g.total; o += (int64_t)gridDim.x * 256) {
    int64_t rem = o, base = 0;
    for (int d = g.rank - 1; d >= 0; --d) {
      const int64_t id = rem % g.n[d];
      rem /= g.n[d];
      base += (id < g.n[d] - g.k[d] ? id : g.n[d] - g.k[d]) * g.stride[d];
    }
    const T* xw = x + base;
    const int64_t r = (g.wsize - 1) / 2;   // lower middle rank
    K v = 0;
    for (int bit = KT::kBits - 1; bit >= 0; --bit) {   // largest v with #{key < v} <= r: the r-th smallest key
      const K t = v | ((K)1 << bit);
      int64_t cnt = 0;
      for (int64_t w = 0; w < g.wsize; ++w) cnt += KT::key(xw[win_off(g, w)]) < t;
      if (cnt <= r) v = t;
    }
    if (g.wsize % 2) {
      out[o] = KT::out(v);
    } else {   // the (r + 1)-th: v again if it repeats, else the next larger key
      int64_t le = 0;
      K nxt = ~(K)0;
      for (int64_t w = 0; w < g.wsize; ++w) {
        const K kk = KT::key(xw[win_off(g, w)]);
        le += kk <= v;
        if (kk > v && kk < nxt) nxt = kk;
      }
      out[o] = KT::mean2(v, le > r + 1 ? v : nxt);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// wiener
struct WienerTail {
  double size;          // window element count
  int32_t has_noise;    // 0: pass 1 (l_var partial sums), 1: apply the formula
  double noise;         // given noise, or
  const double* noise_dev;  // the estimated one (device; read when non-null)
  double* partial;      // pass 1: one sum per workgroup
  int32_t serial;       // the whole tensor is one workgroup: its sum runs in element order (the reference's sequential mean)
};

__device__ __forceinline__ void local_stats(double s1, double s2, double size, double* l_mean, double* l_var) {
  const double m = s1 / size;
  const double m2 = m * m;
  *l_mean = m;
  *l_var = s2 / size - m2;
}

__device__ __forceinline__ double wiener_out(double t, double l_mean, double l_var, double noise) {
  const double q = noise / l_var;
  const double f = 1.0 - q;
  const double d = t - l_mean;
  const double res = d * f;
  return l_var < noise ? l_mean : res + l_mean;
}

// workgroup sum of v (one per thread, in the workgroup's element order) in a fixed order: thread 0 in order when `serial`, else a tree
__device__ __forceinline__ void block_partial(double v, const WienerTail& a) {
  __shared__ double red[256];
  red[threadIdx.x] = v;
  __syncthreads();
  if (a.serial) {
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int q = 0; q < 256; ++q) s += red[q];
      a.partial[blockIdx.x] = s;
    }
    return;
  }
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_wiener_noise(const double* __restrict__ partial, int64_t n_partial, double n_total, double* noise) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t q = threadIdx.x; q < n_partial; q += 256) s += partial[q];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *noise = red[0] / n_total;
}

// wiener.plane: [B][H][W], window KH x KW on the last two axes, tile of 4 rows x 64 columns, one output per thread
constexpr int kWBX = 64, kWBY = 4, kWMaxK = 15;

template <typename T>
__global__ __launch_bounds__(256) void k_wiener_plane(const T* __restrict__ x, T* __restrict__ out, int64_t H, int64_t W, int32_t KH, int32_t KW,
                                                      int64_t tiles_w, int64_t tiles_h, WienerTail a) {
  __shared__ double tile[(kWBY + kWMaxK - 1) * (kWBX + kWMaxK - 1)];
  const int LW = kWBX + KW - 1, LH = kWBY + KH - 1;
  const int lo_h = (KH - 1) - (KH - 1) / 2, lo_w = (KW - 1) - (KW - 1) / 2;
  const int64_t blk = blockIdx.x;
  const int64_t tw = blk % tiles_w, th = (blk / tiles_w) % tiles_h, b = blk / (tiles_w * tiles_h);
  const int64_t r0 = th * kWBY - lo_h, c0 = tw * kWBX - lo_w;
  const T* xb = x + b * H * W;
  for (int e = threadIdx.x; e < LH * LW; e += 256) {
    const int lr = e / LW, lc = e % LW;
    const int64_t gr = r0 + lr, gc = c0 + lc;
    tile[e] = (gr >= 0 && gr < H && gc >= 0 && gc < W) ? (double)xb[gr * W + gc] : 0.0;
  }
  __syncthreads();
  const int tx = threadIdx.x % kWBX, ty = threadIdx.x / kWBX;
  const int64_t i = th * kWBY + ty, j = tw * kWBX + tx;
  const bool live = i < H && j < W;
  double s1 = 0.0, s2 = 0.0;
  if (live) {
    for (int dr = 0; dr < KH; ++dr) {
      const double* row = tile + (ty + dr) * LW + tx;
      for (int dc = 0; dc < KW; ++dc) {
        const double v = row[dc];
        const double v2 = v * v;
        s1 += v;
        s2 += v2;
      }
    }
  }
  double l_mean, l_var;
  local_stats(s1, s2, a.size, &l_mean, &l_var);
  if (!a.has_noise) {
    block_partial(live ? l_var : 0.0, a);
    return;
  }
  if (!live) return;
  const double noise = a.noise_dev ? *a.noise_dev : a.noise;
  out[(b * H + i) * W + j] = (T)wiener_out(tile[(ty + lo_h) * LW + tx + lo_w], l_mean, l_var, noise);
}

template <typename T>
__global__ __launch_bounds__(256) void k_wiener_generic(const T* __restrict__ x, T* __restrict__ out, NdGeom g, WienerTail a) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = o < g.total;
  double s1 = 0.0, s2 = 0.0, t = 0.0;
  if (live) {
    int64_t pos[8];
    int64_t rem = o;
#pragma unroll
    for (int d = 7; d >= 0; --d) {
      if (d < g.rank) {
        pos[d] = rem % g.n[d];
        rem /= g.n[d];
      }
    }
    t = (double)x[o];
    for (int64_t w = 0; w < g.wsize; ++w) {   // row-major over the window; positions in the zero padding add nothing
      int64_t ww = w, off = 0;
      bool in = true;
      for (int q = g.nwin - 1; q >= 0; --q) {
        const int64_t oq = ww % g.wk[q];
        ww /= g.wk[q];
        int64_t p = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d) p = d == g.wax[q] ? pos[d] : p;
        p += oq - g.wlo[q];
        in = in && p >= 0 && p < g.n[g.wax[q]];
        off += (oq - g.wlo[q]) * g.wstride[q];
      }
      if (in) {
        const double v = (double)x[o + off];
        const double v2 = v * v;
        s1 += v;
        s2 += v2;
      }
    }
  }
  double l_mean, l_var;
  local_stats(s1, s2, a.size, &l_mean, &l_var);
  if (!a.has_noise) {
    block_partial(live ? l_var : 0.0, a);
    return;
  }
  if (!live) return;
  const double noise = a.noise_dev ? *a.noise_dev : a.noise;
  out[o] = (T)wiener_out(t, l_mean, l_var, noise);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
template <typename T, int KH, int KW>
hipError_t launch_tile(hipStream_t s, const void* x, float* out, int64_t B, int64_t H, int64_t W) {
  using S = TileShape<KH, KW>;
  const int64_t tiles_w = (W + S::TW - 1) / S::TW, tiles_h = (H + S::TH - 1) / S::TH;
  const int64_t blocks = B * tiles_w * tiles_h;
  if (blocks > 0x7fffffff) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL((k_median_tile<T, KH, KW>), dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const T*>(x), out, H, W, tiles_w, tiles_h);
  return hipGetLastError();
}

template <typename T, int KH, int... KWm1>
hipError_t launch_tile_kw(int kw, hipStream_t s, const void* x, float* out, int64_t B, int64_t H, int64_t W, std::integer_sequence<int, KWm1...>) {
  hipError_t e = hipErrorInvalidValue;
  (void)((kw == KWm1 + 1 ? (e = launch_tile<T, KH, KWm1 + 1>(s, x, out, B, H, W), true) : false) || ...);
  return e;
}

template <typename T, int... KHm1>
hipError_t launch_plane_kh(int kh, int kw, hipStream_t s, const void* x, float* out, int64_t B, int64_t H, int64_t W,
                           std::integer_sequence<int, KHm1...>) {
  hipError_t e = hipErrorInvalidValue;
  (void)((kh == KHm1 + 2 ? (e = launch_tile_kw<T, KHm1 + 2>(kw, s, x, out, B, H, W, std::make_integer_sequence<int, kMedianPlaneMaxK>()), true)
                         : false) || ...);
  return e;
}

int make_geom(const int64_t* shape, int rank, const int64_t* ks, bool wiener, NdGeom* g) {
  *g = NdGeom{};
  g->rank = rank;
  g->total = 1;
  g->wsize = 1;
  int64_t st = 1;
  for (int d = rank - 1; d >= 0; --d) {
    g->n[d] = shape[d];
    g->k[d] = ks[d];
    g->stride[d] = st;
    st *= shape[d];
  }
  g->total = st;
  for (int d = 0; d < rank; ++d) {
    if (ks[d] == 1) continue;
    const int q = g->nwin++;
    g->wk[q] = ks[d];
    g->wstride[q] = g->stride[d];
    g->wlo[q] = wiener ? (ks[d] - 1) - (ks[d] - 1) / 2 : 0;
    g->wax[q] = d;
    g->wsize *= ks[d];
  }
  return NXSIG_OK;
}

// [B][H][W] view of a window that lies on the last two axes (false when another axis has k > 1)
bool plane_view(const int64_t* shape, int rank, const int64_t* ks, int64_t* B, int64_t* H, int64_t* W, int64_t* kh, int64_t* kw) {
  for (int d = 0; d + 2 < rank; ++d)
    if (ks[d] != 1) return false;
  *W = shape[rank - 1];
  *kw = ks[rank - 1];
  *H = rank >= 2 ? shape[rank - 2] : 1;
  *kh = rank >= 2 ? ks[rank - 2] : 1;
  *B = 1;
  for (int d = 0; d + 2 < rank; ++d) *B *= shape[d];
  return true;
}

}  // namespace

int launch_median(Ctx* c, const void* x, bool f64, const int64_t* shape, int rank, const int64_t* ks, float* out) {
  int64_t B, H, W, kh, kw;
  const bool tiles = tune(c, kT_DISABLE_FILTER_TILES, 0) == 0;
  if (tiles && plane_view(shape, rank, ks, &B, &H, &W, &kh, &kw)) {
    if (kh == 1 && kw <= kMedianRowsMaxK) {   // median.rows: every row of the tensor is one row of the view
      dispatch_note("median.rows");
      const hipError_t e = f64 ? launch_tile_kw<double, 1>((int)kw, c->stream, x, out, 1, B * H, W, std::make_integer_sequence<int, kMedianRowsMaxK>())
                               : launch_tile_kw<float, 1>((int)kw, c->stream, x, out, 1, B * H, W, std::make_integer_sequence<int, kMedianRowsMaxK>());
      NXSIG_HIP_TRY(e);
      return NXSIG_OK;
    }
    if (kh <= kMedianPlaneMaxK && kw <= kMedianPlaneMaxK) {
      dispatch_note("median.plane");
      const hipError_t e =
          f64 ? launch_plane_kh<double>((int)kh, (int)kw, c->stream, x, out, B, H, W, std::make_integer_sequence<int, kMedianPlaneMaxK - 1>())
              : launch_plane_kh<float>((int)kh, (int)kw, c->stream, x, out, B, H, W, std::make_integer_sequence<int, kMedianPlaneMaxK - 1>());
      NXSIG_HIP_TRY(e);
      return NXSIG_OK;
    }
  }
  dispatch_note("median.generic");
  NdGeom g;
  make_geom(shape, rank, ks, false, &g);
  const int64_t blocks = (g.total + 255) / 256 < (int64_t)c->num_cus * 64 ? (g.total + 255) / 256 : (int64_t)c->num_cus * 64;
  if (f64) hipLaunchKernelGGL(k_median_generic<double>, dim3((unsigned)blocks), dim3(256), 0, c->stream, static_cast<const double*>(x), out, g);
  else hipLaunchKernelGGL(k_median_generic<float>, dim3((unsigned)blocks), dim3(256), 0, c->stream, static_cast<const float*>(x), out, g);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

int launch_wiener(Ctx* c, const void* x, bool f64, const int64_t* shape, int rank, const int64_t* ks, bool has_noise, double noise, void* out,
                  const double** noise_dev) {
  int64_t B, H, W, kh, kw;
  NdGeom g;
  make_geom(shape, rank, ks, true, &g);
  const bool plane = tune(c, kT_DISABLE_FILTER_TILES, 0) == 0 && plane_view(shape, rank, ks, &B, &H, &W, &kh, &kw) && kh <= kWMaxK && kw <= kWMaxK;
  int64_t blocks;
  int64_t tiles_w = 0, tiles_h = 0;
  if (plane) {
    tiles_w = (W + kWBX - 1) / kWBX;
    tiles_h = (H + kWBY - 1) / kWBY;
    blocks = B * tiles_w * tiles_h;
  } else {
    blocks = (g.total + 255) / 256;
  }
  if (blocks > 0x7fffffff) return set_error(NXSIG_ERR_UNSUPPORTED, "wiener: tensor too large for one launch");
  dispatch_note(plane ? "wiener.plane" : "wiener.generic");
  WienerTail a{};
  a.size = (double)g.wsize;
  a.noise = noise;
  a.has_noise = 1;
  *noise_dev = nullptr;
  auto launch = [&](const WienerTail& t) {
    if (plane) {
      if (f64) hipLaunchKernelGGL(k_wiener_plane<double>, dim3((unsigned)blocks), dim3(256), 0, c->stream, static_cast<const double*>(x),
                                  static_cast<double*>(out), H, W, (int32_t)kh, (int32_t)kw, tiles_w, tiles_h, t);
      else hipLaunchKernelGGL(k_wiener_plane<float>, dim3((unsigned)blocks), dim3(256), 0, c->stream, static_cast<const float*>(x),
                              static_cast<float*>(out), H, W, (int32_t)kh, (int32_t)kw, tiles_w, tiles_h, t);
    } else {
      if (f64) hipLaunchKernelGGL(k_wiener_generic<double>, dim3((unsigned)blocks), dim3(256), 0, c->stream, static_cast<const double*>(x),
                                  static_cast<double*>(out), g, t);
      else hipLaunchKernelGGL(k_wiener_generic<float>, dim3((unsigned)blocks), dim3(256), 0, c->stream, static_cast<const float*>(x),
                              static_cast<float*>(out), g, t);
    }
  };
  if (!has_noise) {   // pass 1, the reduction, then the formula with the estimate
    void* sc = nullptr;
    int rc = ctx_scratch(c, kScratchWienerSums, (size_t)(blocks + 1) * sizeof(double), &sc);
    if (rc) return rc;
    double* noise_cell = static_cast<double*>(sc);
    WienerTail p = a;
    p.has_noise = 0;
    p.partial = noise_cell + 1;
    p.serial = blocks == 1 && (plane ? (B == 1 && H <= kWBY && W <= kWBX) : true);
    launch(p);
    NXSIG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_wiener_noise, dim3(1), dim3(256), 0, c->stream, (const double*)p.partial, blocks, (double)g.total, noise_cell);
    NXSIG_HIP_TRY(hipGetLastError());
    a.noise_dev = noise_cell;
    *noise_dev = noise_cell;
  }
  launch(a);
  NXSIG_HIP_TRY(hipGetLastError());
  return NXSIG_OK;
}

}  // namespace nxsig
