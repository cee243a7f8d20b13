// Record ingest: scipy.signal.savgol_filter(x, wlen, order, mode='interp') along time and ImagingIO's scale
// (modules/imaging_IO.py:37-48) as one pass over the record.
//
// The filter is three host-designed linear maps (das_diff_veh_amd.preprocess.savgol_interp_operator): the taps h
// for the interior and the half x wlen maps el / er of the first / last wlen samples onto the first / last half
// outputs.  A 256-thread block owns a tile of kTile outputs of one row: the tile and its halo go to LDS in the
// record's own type, every lane slides a register window over kRun + wlen - 1 LDS samples for kRun consecutive
// outputs, and the lanes whose run touches a row end replace those outputs by the edge maps (read from global
// memory: 2 half outputs per row); the runs return through LDS so that the block stores whole 16-byte vectors in
// lane order.  Every sum is float64 in tap order j = 0 .. wlen - 1 with one fma per tap, so a
// sample's value does not depend on where its tile, row or stride put it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dvh.h"
#include "dvh_common.h"

using dvh::set_error;

namespace {

constexpr int kThreads = 256;
constexpr int kRun = 8;                   // consecutive outputs per lane
constexpr int kTile = kThreads * kRun;    // outputs per block
constexpr int kMaxWlen = 63;
constexpr int kLdsElems = kTile + kMaxWlen - 1;

// One pad element per 8: a lane's run starts 9 elements after its neighbour's, which spreads the 32 lanes of an LDS
// access group over all banks (float: 9 dwords apart; double: 18, every even bank once).
__device__ __forceinline__ int pad(int i) { return i + (i >> 3); }
constexpr int kLdsPadded = kLdsElems + (kLdsElems >> 3) + 1;

// Wave-uniform load through the scalar cache; the tables are written before the launch.
__device__ __forceinline__ double sld(const double* p) { return *(const __attribute__((address_space(4))) double*)p; }

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

struct Args {
  const void* x;
  void* y;
  int64_t row_stride, y_stride;
  const double *h, *el, *er;
  double divisor;
  int n_t, wlen, n_tiles, x_vec, y_vec;
};

// WLEN: the window length when it is known at compile time (the loop over the taps unrolls and the register window
// slides by renaming), 0: taken from the arguments.
// 8 blocks per CU (at most 64 VGPRs, no scratch): the block's load, filter and store phases do not overlap, so the
// other blocks on the CU cover them; left to itself the unrolled form takes 100+ VGPRs and runs 5-12 % slower.
template <class T, int WLEN>
__global__ __launch_bounds__(kThreads, 8) void savgol_rows_kernel(Args a) {
  __shared__ T lds[kLdsPadded];
  typedef typename Vec16<T>::type V;
  constexpr int NV = Vec16<T>::n;
  const int wlen = WLEN ? WLEN : a.wlen;
  const int half = wlen >> 1;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / a.n_tiles;
  const int tile = blockIdx.x - (int)row * a.n_tiles;
  const int n_t = a.n_t;
  const T* __restrict__ xr = (const T*)a.x + row * a.row_stride;
  T* __restrict__ yr = (T*)a.y + row * a.y_stride;

  // LDS element i holds x[g0 + i], 0 outside the row (only the edge outputs, which the edge maps replace, read it)
  const int g0 = tile * kTile - half;
  const int g1 = g0 + kTile + 2 * half;
  const int lo = g0 > 0 ? g0 : 0;
  const int hi = g1 < n_t ? g1 : n_t;
  const int v0 = g0 >= 0 ? g0 / NV : -((-g0 + NV - 1) / NV);  // floor
  const int v1 = (g1 + NV - 1) / NV;
  // the aligned vectors are all requested before the first one is written to LDS (their latencies overlap)
  constexpr int kIters = ((kTile + kMaxWlen - 1) / NV + 2 + kThreads - 1) / kThreads;
  V q[kIters];
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int e = (v0 + tid + it * kThreads) * NV;
    if (a.x_vec && e >= lo && e + NV <= hi) q[it] = *(const V*)(xr + e);
  }
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int v = v0 + tid + it * kThreads;
    const int e = v * NV;
    if (v >= v1) break;
    if (a.x_vec && e >= lo && e + NV <= hi) {
#pragma unroll
      for (int k = 0; k < NV; ++k) lds[pad(e + k - g0)] = q[it][k];
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int t = e + k;
        if (t >= g0 && t < g1) lds[pad(t - g0)] = (t >= lo && t < hi) ? xr[t] : (T)0;
      }
    }
  }
  __syncthreads();

  const int b = tid * kRun;         // first LDS element of this lane's window
  const int tb = tile * kTile;      // first output of the tile
  const int t0 = tb + b;            // first output of this lane's run
  T out[kRun];
  if (t0 < n_t) {
    double acc[kRun], xw[kRun];
#pragma unroll
    for (int r = 0; r < kRun; ++r) {
      acc[r] = 0.0;
      xw[r] = (double)lds[pad(b + r)];
    }
#pragma unroll
    for (int j = 0; j < wlen; ++j) {
      const double hj = sld(a.h + j);
#pragma unroll
      for (int r = 0; r < kRun; ++r) acc[r] = __builtin_fma(hj, xw[r], acc[r]);
#pragma unroll
      for (int r = 0; r + 1 < kRun; ++r) xw[r] = xw[r + 1];
      xw[kRun - 1] = (double)lds[pad(b + j + kRun)];  // the last one (j = wlen - 1) is inside the array and unused
    }

    // the row's first / last half outputs: the edge maps of its first / last wlen samples
    if (t0 < half || t0 + kRun > n_t - half) {
#pragma unroll
      for (int r = 0; r < kRun; ++r) {
        const int t = t0 + r;
        if (t < n_t && (t < half || t >= n_t - half)) {
          const bool left = t < half;
          const double* m = left ? a.el + t * wlen : a.er + (t - (n_t - half)) * wlen;
          const T* xs = left ? xr : xr + (n_t - wlen);
          double s = 0.0;
          for (int j = 0; j < wlen; ++j) s = __builtin_fma(m[j], (double)xs[j], s);
          acc[r] = s;
        }
      }
    }

#pragma unroll
    for (int r = 0; r < kRun; ++r) out[r] = (T)acc[r];
    if (a.divisor != 1.0) {
      const T d = (T)a.divisor;
#pragma unroll
      for (int r = 0; r < kRun; ++r) out[r] = out[r] / d;
    }
  }

  // the runs go back through LDS (tile element i at pad(i)) so that neighbouring lanes store neighbouring vectors
  __syncthreads();
  if (t0 < n_t) {
#pragma unroll
    for (int r = 0; r < kRun; ++r) lds[pad(b + r)] = out[r];
  }
  __syncthreads();
  const int n_out = n_t - tb < kTile ? n_t - tb : kTile;
#pragma unroll
  for (int it = 0; it < kTile / NV / kThreads; ++it) {
    const int e = (tid + it * kThreads) * NV;
    if (e >= n_out) break;
    if (a.y_vec && e + NV <= n_out) {
      V o;
#pragma unroll
      for (int k = 0; k < NV; ++k) o[k] = lds[pad(e + k)];
      *(V*)(yr + tb + e) = o;
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k)
        if (e + k < n_out) yr[tb + e + k] = lds[pad(e + k)];
    }
  }
}

// x[r][t] /= (T)divisor: ImagingIO's scale on a record that is not smoothed.
template <class T>
__global__ __launch_bounds__(kThreads) void divide_rows_kernel(T* x, int64_t row_stride, int n_t, int64_t total,
                                                               double divisor) {
  const T d = (T)divisor;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / n_t;
    T* p = x + r * row_stride + (i - r * n_t);
    *p = *p / d;
  }
}

}  // namespace

DVH_API int dvh_savgol_rows(const void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t,
                            const double* h, int32_t wlen, const double* el, const double* er, double divisor,
                            void* y, int64_t y_stride, void* stream) {
  if (!x || !y || !h || !el || !er) return set_error(-2, "null pointer argument");
  if (dtype != 0 && dtype != 1) return set_error(-2, "dtype must be 0 (float32) or 1 (float64)");
  if (wlen < 3 || wlen > kMaxWlen || wlen % 2 == 0) return set_error(-4, "window length must be odd, 3 .. 63");
  if (n_t < wlen) return set_error(-4, "rows shorter than the window");
  if (n_t > 0x7fffffff - 2 * kTile) return set_error(-4, "rows too long (the tile arithmetic is 32-bit)");
  if (n_rows < 0 || row_stride < n_t || y_stride < n_t) return set_error(-2, "invalid rows / strides");
  if (!(divisor == divisor) || divisor == 0.0) return set_error(-2, "divisor must be a non-zero number");
  if (n_rows == 0) return 0;
  const int64_t esz = dtype == 0 ? 4 : 8;
  const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
  const uintptr_t xe = xa + (uintptr_t)(((n_rows - 1) * row_stride + n_t) * esz);
  const uintptr_t ye = ya + (uintptr_t)(((n_rows - 1) * y_stride + n_t) * esz);
  if (xa < ye && ya < xe) return set_error(-2, "x and y overlap");
  const int n_tiles = (n_t + kTile - 1) / kTile;
  const int64_t n_blocks = n_rows * n_tiles;
  if (n_blocks > 0x7fffffffLL) return set_error(-4, "too many row tiles for one launch");
  Args a;
  a.x = x;
  a.y = y;
  a.row_stride = row_stride;
  a.y_stride = y_stride;
  a.h = h;
  a.el = el;
  a.er = er;
  a.divisor = divisor;
  a.n_t = n_t;
  a.wlen = wlen;
  a.n_tiles = n_tiles;
  a.x_vec = (xa % 16 == 0 && (row_stride * esz) % 16 == 0) ? 1 : 0;
  a.y_vec = (ya % 16 == 0 && (y_stride * esz) % 16 == 0) ? 1 : 0;
  return dvh::with_float_type(dtype, [&](auto t) {
    using T = decltype(t);
    const dim3 grid((unsigned)n_blocks), block(kThreads);
    if (wlen == 21)
      savgol_rows_kernel<T, 21><<<grid, block, 0, (hipStream_t)stream>>>(a);
    else
      savgol_rows_kernel<T, 0><<<grid, block, 0, (hipStream_t)stream>>>(a);
    return dvh::last_launch();
  });
}

DVH_API int dvh_divide_rows(void* x, int32_t dtype, int64_t n_rows, int64_t row_stride, int32_t n_t, double divisor,
                            void* stream) {
  if (!x) return set_error(-2, "null pointer argument");
  if (dtype != 0 && dtype != 1) return set_error(-2, "dtype must be 0 (float32) or 1 (float64)");
  if (n_rows < 0 || n_t < 0 || row_stride < n_t) return set_error(-2, "invalid rows / strides");
  const int64_t total = n_rows * n_t;
  if (total == 0) return 0;
  int64_t blocks = (total + kThreads - 1) / kThreads;
  const int64_t cap = (int64_t)dvh::cu_count() * 8;
  if (blocks > cap) blocks = cap;
  return dvh::with_float_type(dtype, [&](auto t) {
    using T = decltype(t);
    divide_rows_kernel<T><<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream>>>((T*)x, row_stride, n_t,
                                                                                              total, divisor);
    return dvh::last_launch();
  });
}
