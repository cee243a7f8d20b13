// Vehicle classes on MI355X (gfx950): the quasi-static curve and peak of every pass (the first live cell of the
// imaging notebooks, imaging_diff_speed.ipynb#cell5 / imaging_diff_weight.ipynb#cell7) and the per-class mean and
// std curves (cell 11).
//
//   dvh_qs_curves          curve = detrend(savgol_filter(x.mean(0), wlen, order)), minus its first sample; peak =
//                          max |curve|.  Three launches, all float64:
//     qs_mean_kernel       m[p][t] = (sum_c x[row_off[p][c] + t]) / n_ch into the workspace.  The one pass over the
//                          states: a thread owns 16 bytes of the time axis (2 doubles / 4 floats), the rows are added
//                          in channel order with kRows row loads in flight, one division at the end.
//     qs_savgol_kernel     y = the three Savitzky-Golay maps on m.  Blocks 0 .. n_tiles - 1 of a pass take kTile
//                          interior outputs each from an LDS copy of m with its halo; block n_tiles takes the
//                          2 (wlen / 2) edge outputs from el / er (16 lanes per output), so the interior path holds
//                          no edge product.
//     qs_detrend_kernel    one block per pass: the two sums of the closed-form least-squares line, the curve, its
//                          peak and the pass's status.
//   dvh_class_curve_stats  mean and population std over the passes of every class slot, in pass order.
//
// Determinism: every sum has a fixed order that depends on (n_ch, n_t, wlen) alone -- channel order, tap order in the
// interior, and for the edge outputs and the detrend sums a per-lane strided order followed by a fixed tree.  No block reads another pass and
// there are no atomics, so a pass's curve and peak are the same bits wherever the pass sits in a batch and whether
// its rows come from a batch or from a record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dvh.h"
#include "dvh_common.h"

using dvh::set_error;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = DVH_QS_TILE;        // interior outputs per qs_savgol_kernel block
constexpr int kMaxWlen = DVH_QS_MAX_WLEN;
constexpr int kRows = 8;                  // rows in flight per thread in qs_mean_kernel: 8 x 16 B x 256 = 32 KiB a block
constexpr int kEdgeTaps = (kMaxWlen + 15) / 16;  // taps per lane of an edge output's 16 lanes
static_assert(kTile == 2 * kThreads, "two neighbouring interior outputs per thread");
static_assert(kMaxWlen <= 256, "four taps per lane");

// Wave-uniform load through the scalar cache; the table is written before the launch.
__device__ __forceinline__ int64_t sld(const int64_t* p) {
  return *(const __attribute__((address_space(4))) int64_t*)p;
}

// v of lane `lane` (wave-uniform)
__device__ __forceinline__ double readlane(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// NaN-carrying max (a plain fmax would drop it)
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || a > b) ? a : b; }

template <class T>
struct Vec16;
template <>
struct Vec16<float> {
  typedef float type __attribute__((ext_vector_type(4)));
  static constexpr int n = 4;
};
template <>
struct Vec16<double> {
  typedef double type __attribute__((ext_vector_type(2)));
  static constexpr int n = 2;
};

// 16 bytes from an address that is only element-aligned: one global_load_dwordx4 (global memory takes a wide load at
// dword alignment; a row that starts off a 16-byte boundary costs the wave one more cache line, not narrower loads).
template <class T>
__device__ __forceinline__ typename Vec16<T>::type load16(const T* p) {
  typename Vec16<T>::type v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// m[p][t] for the NV samples from t0 = (chunk * kThreads + tid) * NV on; blockIdx.x = p * n_chunks + chunk.
template <class T>
__global__ __launch_bounds__(kThreads) void qs_mean_kernel(const T* __restrict__ x, const int64_t* __restrict__ row_off,
                                                            int n_ch, int n_t, int n_chunks, double* __restrict__ m) {
  typedef typename Vec16<T>::type V;
  constexpr int NV = Vec16<T>::n;
  const int64_t p = blockIdx.x / n_chunks;
  const int t0 = ((blockIdx.x - (int)p * n_chunks) * kThreads + threadIdx.x) * NV;
  if (t0 >= n_t) return;
  const int64_t* __restrict__ off = row_off + p * n_ch;
  double* __restrict__ mp = m + p * n_t;
  const double div = (double)n_ch;
  if (t0 + NV <= n_t) {
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    int c = 0;
    for (; c + kRows <= n_ch; c += kRows) {
      V v[kRows];
#pragma unroll
      for (int u = 0; u < kRows; ++u) v[u] = load16(x + sld(off + c + u) + t0);
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += (double)v[u][k];
      }
    }
    for (; c < n_ch; ++c) {
      const V v = load16(x + sld(off + c) + t0);
#pragma unroll
      for (int k = 0; k < NV; ++k) acc[k] += (double)v[k];
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) mp[t0 + k] = acc[k] / div;
  } else {  // the row's last, partial vector: element loads, nothing is read past a row's n_t samples
    for (int t = t0; t < n_t; ++t) {
      double acc = 0.0;
      for (int c = 0; c < n_ch; ++c) acc += (double)x[sld(off + c) + t];
      mp[t] = acc / div;
    }
  }
}

// Blocks of a pass: tile k < n_tiles -> interior outputs [k kTile, (k + 1) kTile) cut to [half, n_t - half);
// k == n_tiles (the edge block) -> the 2 half edge outputs.
__global__ __launch_bounds__(kThreads) void qs_savgol_kernel(const double* __restrict__ m, int n_pass, int n_t,
                                                             int n_tiles,
                                                             const double* __restrict__ h, int wlen,
                                                             const double* __restrict__ el,
                                                             const double* __restrict__ er, double* __restrict__ y) {
  __shared__ double lds[kTile + kMaxWlen - 1];
  const int half = wlen >> 1;
  const int tid = threadIdx.x;
  // the first n_pass blocks are the passes' edge blocks (the longest-running ones start first, and consecutive block
  // numbers spread them over every XCD; as block n_tiles of each pass they all fell on two of the eight)
  const bool edge = (int)blockIdx.x < n_pass;
  const int64_t p = edge ? blockIdx.x : (blockIdx.x - n_pass) / n_tiles;
  const int k = edge ? n_tiles : (int)(blockIdx.x - n_pass - p * n_tiles);
  const double* __restrict__ mp = m + p * n_t;
  double* __restrict__ yp = y + p * n_t;
  if (k == n_tiles) {
    // The first and the last wlen samples in LDS, then 16 lanes per output with the taps over them: a row of el / er is
    // read in 128-byte pieces (a thread per output read 64 cache lines per load), its loads are all in flight at once,
    // and the sum has the fixed order "lane l adds taps l, 16 + l, ...; xor tree over the 16 lanes".
    for (int i = tid; i < 2 * wlen; i += kThreads) lds[i] = i < wlen ? mp[i] : mp[n_t - 2 * wlen + i];
    __syncthreads();
    const int sub = tid & 15;
    for (int r = tid >> 4; r < 2 * half; r += kThreads / 16) {
      const double* __restrict__ row = r < half ? el + (int64_t)r * wlen : er + (int64_t)(r - half) * wlen;
      const double* xs = r < half ? lds : lds + wlen;
      double c[kEdgeTaps];
#pragma unroll
      for (int q = 0; q < kEdgeTaps; ++q) c[q] = q * 16 + sub < wlen ? row[q * 16 + sub] : 0.0;
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < kEdgeTaps; ++q)
        if (q * 16 + sub < wlen) s = __builtin_fma(c[q], xs[q * 16 + sub], s);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (sub == 0) yp[r < half ? r : n_t - 2 * half + r] = s;
    }
    return;
  }
  const int tb = k * kTile;
  const int g0 = tb - half;  // lds[i] = m[g0 + i], 0 outside the pass (only outputs the edge block owns read those)
  const int n_lds = kTile + 2 * half;
  for (int i = tid; i < n_lds; i += kThreads) {
    const int t = g0 + i;
    lds[i] = (t >= 0 && t < n_t) ? mp[t] : 0.0;
  }
  __syncthreads();
  // lane l of every wave holds taps l, 64 + l, 128 + l, 192 + l; a tap reaches the wave by readlane (a scalar load per
  // tap made the loop wait out a scalar-cache round trip 101 times)
  double hv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) hv[q] = q * 64 + (tid & 63) < wlen ? h[q * 64 + (tid & 63)] : 0.0;
  // the thread's two outputs are neighbours (tile elements 2 tid and 2 tid + 1): their windows overlap in all but one
  // sample, so a tap costs one LDS read
  double a0 = 0.0, a1 = 0.0;
  double w0 = lds[2 * tid];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int nj = wlen - q * 64 < 64 ? wlen - q * 64 : 64;
    for (int jj = 0; jj < nj; ++jj) {
      const double hj = readlane(hv[q], jj);
      const double w1 = lds[2 * tid + q * 64 + jj + 1];
      a0 = __builtin_fma(hj, w0, a0);
      a1 = __builtin_fma(hj, w1, a1);
      w0 = w1;
    }
  }
  const int ta = tb + 2 * tid, tc = ta + 1;
  if (ta >= half && ta < n_t - half) yp[ta] = a0;
  if (tc >= half && tc < n_t - half) yp[tc] = a1;
}

// block sum in a fixed order: xor tree inside a wave, then the waves in order
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) s += sh[w];
  return s;
}

// scipy.signal.detrend(y) (type='linear': least squares on [(t + 1) / n_t, 1]) in closed form, with a[t] = (t + 1) /
// n_t, abar = (n_t + 1) / (2 n_t) and sum (a - abar)^2 = (n_t^2 - 1) / (12 n_t):
//   slope = sum (a[t] - abar) y[t] / sum (a - abar)^2,  icpt = sum y[t] / n_t - slope abar,  z = y - (slope a + icpt)
// then curve = z - z[0] and the peak.  One block per pass.
__global__ __launch_bounds__(kThreads) void qs_detrend_kernel(const double* __restrict__ y, int n_t,
                                                              double* __restrict__ curves, int64_t curve_stride,
                                                              double* __restrict__ peaks, int32_t* __restrict__ status) {
  __shared__ double sh[kThreads / 64];
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x;
  const double* __restrict__ yp = y + p * n_t;
  const double n = (double)n_t;
  const double abar = (n + 1.0) / (2.0 * n);
  double s0 = 0.0, s1 = 0.0;
  for (int t = tid; t < n_t; t += kThreads) {
    const double v = yp[t];
    const double a = (double)(t + 1) / n;
    s0 += v;
    s1 = __builtin_fma(a - abar, v, s1);
  }
  s0 = block_sum(s0, sh);
  s1 = block_sum(s1, sh);
  const double slope = s1 / ((n * n - 1.0) / (12.0 * n));
  const double icpt = s0 / n - slope * abar;
  const double z0 = yp[0] - __builtin_fma(slope, 1.0 / n, icpt);
  double* __restrict__ cp = curves ? curves + p * curve_stride : nullptr;
  double pk = 0.0;
  int bad = 0;
  for (int t = tid; t < n_t; t += kThreads) {
    const double a = (double)(t + 1) / n;
    const double c = (yp[t] - __builtin_fma(slope, a, icpt)) - z0;
    if (cp) cp[t] = c;
    const double ac = fabs(c);
    bad |= !(ac <= 1.79769313486231570815e308);  // NaN or inf
    pk = nan_max(pk, ac);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    pk = nan_max(pk, __shfl_xor(pk, o));
    bad |= __shfl_xor(bad, o);
  }
  __shared__ int shb[kThreads / 64];
  __syncthreads();
  if ((tid & 63) == 0) {
    sh[tid >> 6] = pk;
    shb[tid >> 6] = bad;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {
      pk = nan_max(pk, sh[w]);
      bad |= shb[w];
    }
    peaks[p] = bad ? __builtin_nan("") : pk;
    if (bad && status) status[p] |= 1;
  }
}

// np.mean / np.std (population, two passes) over the passes of slot blockIdx.y, per sample, in pass order.  The
// products are not contracted into the sums: NumPy squares, then adds.
__global__ __launch_bounds__(kThreads) void class_stats_kernel(const double* __restrict__ curves, int64_t curve_stride,
                                                               const int32_t* __restrict__ slots, int n_pass, int n_t,
                                                               double* __restrict__ mean, double* __restrict__ sd,
                                                               int32_t* __restrict__ count) {
#pragma clang fp contract(off)
  constexpr int U = 8;
  const int s = blockIdx.y;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= n_t) return;
  const double* __restrict__ col = curves + t;
  double sum = 0.0;
  int n = 0;
  for (int p0 = 0; p0 < n_pass; p0 += U) {
    double v[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      in[u] = p0 + u < n_pass && slots[p0 + u] == s;
      v[u] = in[u] ? col[(int64_t)(p0 + u) * curve_stride] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (in[u]) {
        sum += v[u];
        ++n;
      }
  }
  const double mu = sum / (double)n;  // 0 / 0 = NaN for an empty slot, as NumPy
  double ss = 0.0;
  for (int p0 = 0; p0 < n_pass; p0 += U) {
    double v[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      in[u] = p0 + u < n_pass && slots[p0 + u] == s;
      v[u] = in[u] ? col[(int64_t)(p0 + u) * curve_stride] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (in[u]) {
        const double d = v[u] - mu;
        const double d2 = d * d;
        ss += d2;
      }
  }
  mean[(int64_t)s * n_t + t] = mu;
  sd[(int64_t)s * n_t + t] = sqrt(ss / (double)n);
  if (t == 0) count[s] = n;
}

}  // namespace

DVH_API int64_t dvh_qs_curves_workspace(int32_t n_pass, int32_t n_t) {
  if (n_pass <= 0 || n_t <= 0) return 0;
  return 2 * (int64_t)n_pass * n_t * (int64_t)sizeof(double);
}

DVH_API int dvh_qs_curves(const void* x, int32_t dtype, const int64_t* row_off, int32_t n_pass, int32_t n_ch,
                          int32_t n_t, const double* h, int32_t wlen, const double* el, const double* er,
                          double* curves, int64_t curve_stride, double* peaks, int32_t* status, void* ws,
                          void* stream) {
  if (dtype != 0 && dtype != 1) return set_error(-2, "dtype must be 0 (float32) or 1 (float64)");
  if (wlen < 3 || wlen > kMaxWlen || wlen % 2 == 0) return set_error(-4, "window length must be odd, 3 .. 255");
  if (n_t < wlen) return set_error(-4, "passes shorter than the window");
  if (n_ch < 1) return set_error(-4, "a pass needs at least one channel");
  if (n_pass < 0) return set_error(-4, "negative number of passes");
  if (n_t > 0x7fffffff - 2 * kTile) return set_error(-4, "passes too long (the tile arithmetic is 32-bit)");
  if (n_pass == 0) return 0;
  if (!x || !row_off || !h || !el || !er || !peaks || !ws) return set_error(-2, "null pointer argument");
  if (curves && curve_stride < n_t) return set_error(-2, "curve_stride shorter than a curve");
  if ((uintptr_t)x % (dtype == 0 ? 4 : 8)) return set_error(-2, "x is not aligned to its element size");
  const int n_tiles = (n_t + kTile - 1) / kTile;
  if ((int64_t)n_pass * (n_tiles + 1) > 0x7fffffffLL) return set_error(-4, "too many tiles for one launch");
  hipStream_t s = (hipStream_t)stream;
  double* m = (double*)ws;
  double* y = m + (int64_t)n_pass * n_t;
  const int rc = dvh::with_float_type(dtype, [&](auto t) {
    using T = decltype(t);
    constexpr int per_block = kThreads * (16 / (int)sizeof(T));
    const int n_chunks = (n_t + per_block - 1) / per_block;
    qs_mean_kernel<T><<<dim3((unsigned)(n_pass * n_chunks)), dim3(kThreads), 0, s>>>((const T*)x, row_off, n_ch, n_t,
                                                                                     n_chunks, m);
    return 0;
  });
  if (rc) return rc;
  qs_savgol_kernel<<<dim3((unsigned)(n_pass * (n_tiles + 1))), dim3(kThreads), 0, s>>>(m, n_pass, n_t, n_tiles, h, wlen,
                                                                                     el, er, y);
  qs_detrend_kernel<<<dim3((unsigned)n_pass), dim3(kThreads), 0, s>>>(y, n_t, curves, curve_stride, peaks, status);
  return dvh::last_launch();
}

DVH_API int dvh_class_curve_stats(const double* curves, int64_t curve_stride, const int32_t* slots, int32_t n_pass,
                                  int32_t n_t, int32_t n_slot, double* mean, double* std, int32_t* count,
                                  void* stream) {
  if (n_pass < 0 || n_t < 1 || n_slot < 0 || n_slot > 65535) return set_error(-4, "invalid sizes");
  if (n_slot == 0) return 0;
  if (!mean || !std || !count || (n_pass > 0 && (!curves || !slots))) return set_error(-2, "null pointer argument");
  if (curve_stride < n_t) return set_error(-2, "curve_stride shorter than a curve");
  class_stats_kernel<<<dim3((unsigned)((n_t + kThreads - 1) / kThreads), (unsigned)n_slot), dim3(kThreads), 0,
                       (hipStream_t)stream>>>(curves, curve_stride, slots, n_pass, n_t, mean, std, count);
  return dvh::last_launch();
}
